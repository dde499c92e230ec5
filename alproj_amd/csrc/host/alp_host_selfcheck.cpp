// Self-checking driver of the HIP-free host code (host/alp_host.h, host/alp_host.cpp, host/alp_buffer.h).  NOT part of libalproj_hip.so:
// alproj_amd/_build.py: build_host() links it with alp_host.cpp into build/host_san/alp_host_{plain,asan,tsan} and
// tests/test_host_sanitized.py runs the three executables.  Every threaded helper is called with sizes that straddle
// its thread thresholds (1, 70 001, one short of / exactly / one past a slice, two slices and a ragged rest), with
// thread counts from 1 to 64, from several caller threads at once (independent handles may be used concurrently:
// include/alproj_hip.h), and compared with a serial restatement written here.  Exit code 0 and "host selfcheck ok" =
// every comparison held; the sanitizers add their own verdict on stderr.  --plan prints what host/alp_plan.h plans for the
// queries it is given (tests/test_launch_plan.py holds the Python restatements of the launch rules to it, and reads the render
// frame's plans and overflow verdicts off it); --lm runs the Levenberg-Marquardt state machine of host/alp_lm.h on sums read from
// stdin (tests/test_lm_device_host.py holds it to alproj_amd/optimize.py: _normal_lm_steps).
#include <cinttypes>
#include <mutex>
#include <random>
#include <string>
#include <utility>

#include "host/alp_host.h"
#include "host/alp_buffer.h"

using namespace alp;

namespace {

std::atomic<int> g_failures{0};
std::mutex g_print;

#define CHECK(cond, ...)                                           \
    do {                                                           \
        if (!(cond)) {                                             \
            std::lock_guard<std::mutex> lk(g_print);               \
            fprintf(stderr, "CHECK FAILED %s:%d: %s | ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                          \
            fprintf(stderr, "\n");                                 \
            g_failures.fetch_add(1);                               \
        }                                                          \
    } while (0)

const int THREAD_COUNTS[] = {1, 2, 3, 7, 16, 64};

// ------------------------------------------------------------------ alp_host_hash64
void check_hash() {
    const int64_t SL = host::HASH_SLICE_BYTES;
    const int64_t sizes[] = {0, 1, 7, 8, 31, 32, 33, 70001, SL - 1, SL, SL + 1, 2 * SL + 12345};
    std::vector<unsigned char> buf((size_t)(2 * SL + 12345) + 3);
    std::mt19937_64 rng(1);
    for (auto &b : buf) b = (unsigned char)rng();
    for (int shift = 0; shift < 2; ++shift)                    // an aligned and an odd start address
        for (int64_t n : sizes) {
            uint64_t d1 = 0;
            CHECK(alp_host_hash64(buf.data() + shift, n, 1, &d1) == ALP_OK, "n=%" PRId64, n);
            for (int T : THREAD_COUNTS) {
                uint64_t d = 0;
                CHECK(alp_host_hash64(buf.data() + shift, n, T, &d) == ALP_OK, "n=%" PRId64, n);
                CHECK(d == d1, "digest depends on the thread count: n=%" PRId64 " T=%d", n, T);
            }
            uint64_t d0 = 0;
            CHECK(alp_host_hash64(buf.data() + shift, n, 0, &d0) == ALP_OK && d0 == d1, "default thread count, n=%" PRId64, n);
            if (n > 0) {                                        // one changed byte (first, last) always changes the digest
                for (int64_t at : {(int64_t)0, n - 1}) {
                    buf[(size_t)(shift + at)] ^= 0x40;
                    uint64_t d = 0;
                    alp_host_hash64(buf.data() + shift, n, 3, &d);
                    CHECK(d != d1, "changed byte %" PRId64 " of %" PRId64 " not seen", at, n);
                    buf[(size_t)(shift + at)] ^= 0x40;
                }
            }
        }
    uint64_t d = 0;
    CHECK(alp_host_hash64(nullptr, 8, 1, &d) == ALP_EINVAL, "NULL buffer accepted");
    CHECK(alp_host_hash64(buf.data(), -1, 1, &d) == ALP_EINVAL, "negative size accepted");
    CHECK(alp_host_hash64(buf.data(), 8, 1, nullptr) == ALP_EINVAL, "NULL digest accepted");
    CHECK(strstr(alp_last_error(), "alp_host_hash64") != nullptr, "error text: %s", alp_last_error());
}

// ------------------------------------------------------------------ alp_host_minmax
void check_minmax() {
    const int64_t per = host::MINMAX_VALUES_PER_THREAD;
    const int64_t sizes[] = {1, 7, 8, 9, 70001, per - 1, per, per + 1, 2 * per + 77777};
    std::vector<double> v((size_t)(2 * per + 77777));
    std::mt19937_64 rng(2);
    std::uniform_real_distribution<double> U(-1e6, 1e6);
    for (auto &x : v) x = U(rng);
    for (int64_t n : sizes) {
        double lo = INFINITY, hi = -INFINITY;
        for (int64_t i = 0; i < n; ++i) { lo = std::min(lo, v[(size_t)i]); hi = std::max(hi, v[(size_t)i]); }
        for (int T : {0, 1, 2, 3, 8, 64}) {
            double out[2] = {0, 0};
            CHECK(alp_host_minmax(v.data(), n, T, out) == ALP_OK, "n=%" PRId64, n);
            CHECK(out[0] == lo && out[1] == hi, "n=%" PRId64 " T=%d: %g %g vs %g %g", n, T, out[0], out[1], lo, hi);
        }
        // a NaN anywhere (first value, last value, the first value of the second thread's share) poisons both
        for (int64_t at : {(int64_t)0, n - 1, n / 2}) {
            const double keep = v[(size_t)at];
            v[(size_t)at] = NAN;
            for (int T : {1, 2, 8}) {
                double out[2] = {0, 0};
                alp_host_minmax(v.data(), n, T, out);
                CHECK(out[0] != out[0] && out[1] != out[1], "NaN at %" PRId64 " of %" PRId64 " lost (T=%d)", at, n, T);
            }
            v[(size_t)at] = keep;
        }
    }
    double out[2];
    CHECK(alp_host_minmax(v.data(), 0, 1, out) == ALP_EINVAL, "n = 0 accepted");
    CHECK(alp_host_minmax(nullptr, 4, 1, out) == ALP_EINVAL, "NULL accepted");
}

// ------------------------------------------------------------------ alp_host_prefault
void check_prefault() {
    const int64_t sizes[] = {0, 1, 4095, 4096, 4097, 70001, (5 << 20) + 3, 9 << 20};
    for (int64_t n : sizes)
        for (int shift : {0, 1, 4095})
            for (int T : {0, 1, 4, 64}) {
                std::vector<unsigned char> buf((size_t)(n + shift) + 1, 0xA5);
                CHECK(alp_host_prefault(buf.data() + shift, n, T) == ALP_OK, "n=%" PRId64, n);
                // populated pages keep their contents (MADV_POPULATE_WRITE faults them in, it does not clear them)
                bool same = true;
                for (unsigned char b : buf) same &= b == 0xA5;
                CHECK(same, "prefault changed the buffer: n=%" PRId64 " shift=%d T=%d", n, shift, T);
            }
    CHECK(alp_host_prefault(nullptr, 16, 1) == ALP_EINVAL, "NULL accepted");
    CHECK(alp_host_prefault(nullptr, 0, 1) == ALP_OK, "empty range refused");
}

// ------------------------------------------------------------------ fold_pose against the unfolded arithmetic
// optimize.py:35-38 (intrinsic_mat), :71-95 (extrinsic_mat), :144-149 (project), :104-106 (_distort's centring), written
// out matrix by matrix as the reference has it; the folded record must give the same normalised coordinates.
void check_fold_pose() {
    std::mt19937_64 rng(3);
    std::uniform_real_distribution<double> U(-1, 1);
    for (int trial = 0; trial < 200; ++trial) {
        double p[ALP_NPARAM] = {0};
        const double origin[3] = {732000 + 100 * U(rng), 4048000 + 100 * U(rng), 2000 + 10 * U(rng)};
        p[0] = origin[0] + 500 * U(rng); p[1] = origin[1] + 500 * U(rng); p[2] = origin[2] + 200 * U(rng);
        p[3] = 60 + 25 * U(rng); p[4] = 180 * U(rng); p[5] = 30 * U(rng); p[6] = 10 * U(rng);
        for (int i = 7; i < 21; ++i) p[i] = 0.1 * U(rng);
        p[21] = 5616; p[22] = 3744; p[23] = 2808 + 50 * U(rng); p[24] = 1872 + 50 * U(rng);
        double rec[POSE_WORDS];
        fold_pose(p, origin, rec);
        PoseRec<float> rf;
        fold_pose_t<float>(p, origin, &rf);
        for (int i = 0; i < POSE_WORDS; ++i) CHECK(rf.v[i] == (float)rec[i], "fold_pose_t word %d", i);
        CHECK(rec[18] == 1 + p[7] && rec[19] == 1 + p[8] && rec[20] == 2 * p[15] && rec[21] == 2 * p[16], "coefficients");
        const double pi = M_PI, w = p[21], h = p[22];
        const double fovx = p[3] * pi / 180, fovy = fovx * h / w;
        const double fx = w / (2 * std::tan(fovx / 2)), fy = h / (2 * std::tan(fovy / 2));
        const double a = p[4] * pi / 180, b = -(p[5] + 90) * pi / 180, c = -p[6] * pi / 180;
        const double Rz[3][3] = {{cos(a), -sin(a), 0}, {sin(a), cos(a), 0}, {0, 0, 1}};
        const double Rx[3][3] = {{1, 0, 0}, {0, cos(b), -sin(b)}, {0, sin(b), cos(b)}};
        const double Ry[3][3] = {{cos(c), 0, sin(c)}, {0, 1, 0}, {-sin(c), 0, cos(c)}};
        double M[3][3] = {{0}}, R[3][3] = {{0}};
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) M[i][j] += Rx[i][k] * Ry[k][j];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) R[i][j] += M[i][k] * Rz[k][j];
        const double c0 = (double)(float)((w - 1) / 2), c1 = (double)(float)((h - 1) / 2);
        for (int k = 0; k < 8; ++k) {
            const double q[3] = {2000 * U(rng), 2000 * U(rng), 300 * U(rng)};       // local coordinates
            const double P[3] = {origin[0] + q[0] - p[0], origin[1] + q[1] - p[1], origin[2] + q[2] - p[2]};
            double cam[3];
            for (int i = 0; i < 3; ++i) cam[i] = R[i][0] * P[0] + R[i][1] * P[1] + R[i][2] * P[2];
            const double x = fx * cam[0] + p[23] * cam[2], y = fy * cam[1] + p[24] * cam[2], z = cam[2];
            const double x1 = ((w - x / z) - c0) / c0, y1 = (y / z - c1) / c1;
            const double zf = rec[8] * q[0] + rec[9] * q[1] + rec[10] * q[2] + rec[11];
            const double x1f = (rec[0] * q[0] + rec[1] * q[1] + rec[2] * q[2] + rec[3]) / zf;
            const double y1f = (rec[4] * q[0] + rec[5] * q[1] + rec[6] * q[2] + rec[7]) / zf;
            if (std::fabs(z) < 1) continue;                    // next to the camera plane the quotient amplifies rounding
            CHECK(std::fabs(x1f - x1) <= 1e-9 * std::max(1.0, std::fabs(x1)), "x1 %.17g vs %.17g", x1f, x1);
            CHECK(std::fabs(y1f - y1) <= 1e-9 * std::max(1.0, std::fabs(y1)), "y1 %.17g vs %.17g", y1f, y1);
            // the lens-free folding of the same pose with its lens coefficients set to zero: optimize.py:112-118 is then
            // u = c0 x1 + c0, v = c1 y1 (1 + a1) / (1 + a2) + c1, and the folded rows give the residual against any (uo, vo)
            double pl[ALP_NPARAM];
            memcpy(pl, p, sizeof(pl));
            for (int i = 9; i <= 20; ++i) pl[i] = 0;
            CHECK(pose_is_lens_free(pl) && !pose_is_lens_free(p), "pose_is_lens_free");
            double lf[POSE_WORDS];
            fold_pose_lens_free(pl, origin, lf);
            const double uo = 5616 * U(rng), vo = 3744 * U(rng);
            const double u_ref = c0 * x1 + c0, v_ref = c1 * (y1 * (1 + pl[7]) / (1 + pl[8])) + c1;
            const double zl = lf[8] * q[0] + lf[9] * q[1] + lf[10] * q[2] + lf[11];
            const double du = (uo - lf[26]) + (lf[0] * q[0] + lf[1] * q[1] + lf[2] * q[2] + lf[3]) / zl;
            const double dv = (vo - lf[27]) + (lf[4] * q[0] + lf[5] * q[1] + lf[6] * q[2] + lf[7]) / zl;
            CHECK(std::fabs(du - (uo - u_ref)) <= 1e-8 * std::max(1.0, std::fabs(u_ref)), "lens-free du %.17g vs %.17g", du, uo - u_ref);
            CHECK(std::fabs(dv - (vo - v_ref)) <= 1e-8 * std::max(1.0, std::fabs(v_ref)), "lens-free dv %.17g vs %.17g", dv, vo - v_ref);
            CHECK(zl == zf && lf[26] == c0 && lf[27] == c1 && lf[12] == 0 && lf[31] == 0, "lens-free record layout");
        }
    }
}

// ------------------------------------------------------------------ conversion workers of the converting fetch
template <typename S, typename D>
void check_convert_t() {
    const int64_t lim = host::CONVERT_SERIAL_BELOW;
    const int64_t sizes[] = {0, 1, 15, 16, 17, lim - 1, lim, lim + 1, 70001, (1 << 20) + 3};
    std::mt19937_64 rng(4);
    std::uniform_real_distribution<double> U(-1e7, 1e7);
    for (int64_t n : sizes) {
        std::vector<S> src((size_t)n);                          // exactly n: a sanitizer sees one value too many on either side
        for (auto &x : src) x = (S)U(rng);
        for (int T : THREAD_COUNTS) {
            std::vector<D> dst((size_t)n, (D)-1);
            host::convert_threads(src.data(), dst.data(), n, T);
            bool same = true;
            for (int64_t i = 0; i < n; ++i) same &= dst[(size_t)i] == (D)src[(size_t)i];
            CHECK(same, "convert n=%" PRId64 " T=%d", n, T);
        }
    }
}

void check_convert() {
    check_convert_t<float, double>();
    check_convert_t<double, float>();
}

// ------------------------------------------------------------------ regular-grid recognition
template <typename I>
std::vector<I> grid_indices(long long gh, long long gw) {       // surface.py:194-201
    std::vector<I> ind;
    ind.reserve((size_t)((gh - 1) * (gw - 1) * 6));
    for (long long r = 0; r + 1 < gh; ++r)
        for (long long c = 0; c + 1 < gw; ++c) {
            const long long a = r * gw + c;
            for (long long v : {a, a + gw, a + gw + 1, a, a + gw + 1, a + 1}) ind.push_back((I)v);
        }
    return ind;
}

template <typename I>
void check_grid_t(int dtype) {
    const long long shapes[][2] = {{2, 2}, {3, 5}, {17, 4}, {2, 300}, {300, 251}};
    for (auto &sh : shapes) {
        const long long gh = sh[0], gw = sh[1];
        std::vector<I> ind = grid_indices<I>(gh, gw);
        const int64_t n_tri = (int64_t)ind.size() / 3, n_vert = gh * gw;
        long long cgh = 0, cgw = 0;
        CHECK(host::grid_candidate(ind.data(), dtype, n_tri, n_vert, &cgh, &cgw) && cgh == gh && cgw == gw, "candidate %lld x %lld", gh, gw);
        CHECK(!host::grid_candidate(ind.data(), dtype, n_tri - 1, n_vert, &cgh, &cgw), "odd triangle count accepted");
        CHECK(!host::grid_candidate(ind.data(), dtype, n_tri, n_vert + 1, &cgh, &cgw) || (n_vert + 1) % gw == 0, "wrong vertex count accepted");
        for (int T : {1, 2, 8, 64}) {
            {
                host::HostGridCheck chk;
                chk.start(ind.data(), dtype, gh, gw, T);
                CHECK(chk.is_grid(), "grid %lld x %lld not recognised (T=%d)", gh, gw, T);
            }
            for (size_t at : {(size_t)0, ind.size() / 2, ind.size() - 1}) {     // one wrong entry anywhere
                const I keep = ind[at];
                ind[at] = (I)(keep + 1);
                {
                    host::HostGridCheck chk;
                    chk.start(ind.data(), dtype, gh, gw, T);
                    CHECK(!chk.is_grid(), "wrong entry %zu of a %lld x %lld grid not seen (T=%d)", at, gh, gw, T);
                }
                ind[at] = keep;
            }
            {                                                   // leaving the scope without asking: the destructor stops and joins
                host::HostGridCheck chk;
                chk.start(ind.data(), dtype, gh, gw, T);
            }
            {                                                   // never started
                host::HostGridCheck chk;
                CHECK(!chk.is_grid(), "a check that never ran says grid");
            }
        }
    }
}

void check_grid() {
    check_grid_t<int>(ALP_I32);
    check_grid_t<long long>(ALP_I64);
}

// ------------------------------------------------------------------ argmin and confirmation band
void check_selection() {
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> U(0, 1);
    for (int trial = 0; trial < 400; ++trial) {
        const int64_t P = 1 + (int64_t)(rng() % 300);
        const double n_total = 1000;
        std::vector<double> sums((size_t)P), loss((size_t)P);
        const int mode = trial % 5;
        for (int64_t i = 0; i < P; ++i) {
            double l = 10 + U(rng);                                              // mode 0: well separated
            if (mode == 1) l = 10 * (1 + 1e-5 * U(rng));                         // everything inside the band
            if (mode == 2 && rng() % 3 == 0) l = NAN;                            // NaNs in between
            if (mode == 3) l = (double)(1 + rng() % 3);                          // many exact ties
            if (mode == 4) l = NAN;                                              // all NaN
            sums[(size_t)i] = l * n_total;
        }
        double best_v = 0;
        const int64_t best = host::losses_and_argmin(sums.data(), P, n_total, loss.data(), &best_v);
        int64_t want = -1;
        for (int64_t i = 0; i < P; ++i)
            if (loss[(size_t)i] == loss[(size_t)i] && (want < 0 || loss[(size_t)i] < loss[(size_t)want])) want = i;
        CHECK(best == want, "argmin %" PRId64 " vs %" PRId64, best, want);
        if (best < 0) continue;
        CHECK(best_v == loss[(size_t)best], "best value");
        int64_t which[host::CONFIRM_MAX];
        int K = 0;
        const int64_t in_band = host::confirm_band(loss.data(), P, best_v, which, &K);
        std::vector<int64_t> band;
        for (int64_t i = 0; i < P; ++i)
            if (loss[(size_t)i] <= best_v + host::CONFIRM_GAP * std::fabs(best_v)) band.push_back(i);
        CHECK(in_band == (int64_t)band.size(), "band size");
        CHECK(K == (int)std::min<size_t>(band.size(), host::CONFIRM_MAX), "K");
        for (int k = 1; k < K; ++k) CHECK(which[k - 1] < which[k], "which[] not ascending");
        // the kept ones are the K smallest of the band: nothing left out is smaller than something kept
        double kept_max = -INFINITY;
        for (int k = 0; k < K; ++k) kept_max = std::max(kept_max, loss[(size_t)which[k]]);
        for (int64_t i : band)
            if (!std::binary_search(which, which + K, i)) CHECK(loss[(size_t)i] >= kept_max, "a smaller candidate was left out of the band");
        CHECK(std::binary_search(which, which + K, best), "the float32 argmin is not in its own band");
        // confirmation: float64 sums reorder the band
        std::vector<double> csums((size_t)K + 1);
        for (int k = 0; k < K; ++k) csums[(size_t)k] = (mode == 2 && k % 2 ? NAN : U(rng)) * n_total;
        csums[(size_t)K] = n_total;
        const int64_t cbest = host::merge_confirmed(loss.data(), which, K, csums.data());
        int64_t cwant = -1;
        double cwant_v = 0;
        for (int k = 0; k < K; ++k) {
            const double l = csums[(size_t)k] / n_total, stored = loss[(size_t)which[k]];
            CHECK(stored == l || (l != l && stored != stored), "confirmed loss not stored");
            if (l == l && (cwant < 0 || l < cwant_v)) { cwant = which[k]; cwant_v = l; }
        }
        CHECK(cbest == (cwant < 0 ? which[0] : cwant), "confirmed argmin");
    }
}

// ------------------------------------------------------------------ launch planning (host/alp_plan.h)
// invariants of every plan over point counts around whole rows of 256, populations from one candidate to the ABI's limit, both
// precisions with their two group heights, small and large GPUs; tests/test_launch_plan.py compares single plans (--plan)
void check_plan() {
    std::vector<int64_t> ns = {1, 2, 300, 1127, 67 * 256 - 37, 100000, 1000000, 10000000, 30000000, 100000000};
    for (int64_t k : {1, 2, 5, 24, 1024, 4096, 39063, 390625})
        for (int64_t d : {-1, 0, 1}) ns.push_back(k * 256 + d);
    const int64_t Ps[] = {1, 2, 127, 128, 129, 250, 256, 384, 2048, 4096, 8192, 32768, 65536, (int64_t)1 << 20};
    const int TC = 128;
    for (int cu : {1, 64, 256, 304})
        for (int64_t n : ns) {
            const int64_t rows = (n + 255) / 256;
            const int sg = host::stream_grid(n, cu), cg = host::confirm_grid(n, cu);
            CHECK(sg >= 1 && sg <= 8 * cu && (sg == 8 * cu || sg == rows), "stream_grid(%" PRId64 ", %d) = %d", n, cu, sg);
            CHECK(cg >= 1 && cg <= 4 * cu && cg <= rows, "confirm_grid(%" PRId64 ", %d) = %d", n, cu, cg);
            for (int64_t P : Ps)
                for (int f64 = 0; f64 < 2; ++f64)
                    for (int V : {f64 ? 5 : 6, f64 ? 6 : 8})
                        for (int batched = 0; batched < 2; ++batched) {
                            const int64_t tiles = (P + TC - 1) / TC;
                            const host::PopGrid g = host::pop_grid(n, P, f64, V, TC, cu, batched);
                            CHECK(g.stripes >= 1 && g.stripes <= rows && g.tile_cols >= 1 && g.tile_cols <= tiles,
                                  "pop_grid(%" PRId64 ", %" PRId64 ", f64=%d, V=%d, cu=%d, batched=%d) = %d x %d", n, P, f64, V, cu, batched,
                                  g.stripes, g.tile_cols);
                            CHECK(!batched || (int64_t)g.stripes * P * 8 <= host::POP_BATCHED_PARTIALS_BYTES,
                                  "batched partial sums: %d stripes x %" PRId64, g.stripes, P);
                            // ALP_POP_GRID: a valid pair is taken (stripes still clamped to the rows), any other one ignored
                            const int64_t want_rows = std::min<int64_t>(rows, 7);
                            const host::PopGrid o = host::pop_grid(n, P, f64, V, TC, cu, false, 7, (int)tiles);
                            CHECK(o.stripes == want_rows && o.tile_cols == tiles, "override 7 x %" PRId64 " -> %d x %d", tiles, o.stripes, o.tile_cols);
                            const host::PopGrid big = host::pop_grid(n, P, f64, V, TC, cu, batched, 1 << 30, 1);
                            CHECK(big.stripes >= 1 && big.stripes <= rows && big.tile_cols >= 1 && big.tile_cols <= tiles, "override 2^30 x 1");
                            const host::PopGrid none = host::pop_grid(n, P, f64, V, TC, cu, false);
                            for (auto &bad : {std::pair<int, int>{0, 1}, {3, 0}, {3, (int)tiles + 1}, {-2, 1}}) {
                                const host::PopGrid i = host::pop_grid(n, P, f64, V, TC, cu, false, bad.first, bad.second);
                                CHECK(i.stripes == none.stripes && i.tile_cols == none.tile_cols, "override %d,%d not ignored", bad.first, bad.second);
                            }
                        }
            // mend_grid: planned for all P candidates -- the tile columns cover them, the stripes are rows, the partial rows fit
            for (int64_t P : Ps) {
                const host::PopGrid m = host::mend_grid(n, P, 5, TC, cu);
                CHECK(m.stripes >= 1 && m.stripes <= rows && (int64_t)m.tile_cols * TC >= P && (int64_t)(m.tile_cols - 1) * TC < P,
                      "mend_grid(%" PRId64 ", %" PRId64 ", cu=%d) = %d x %d", n, P, cu, m.stripes, m.tile_cols);
                CHECK((int64_t)m.stripes * P * 8 <= host::POP_BATCHED_PARTIALS_BYTES, "mend partial sums: %d stripes x %" PRId64, m.stripes, P);
            }
            for (int64_t pairs : {1, 2, 3, 11, 21, 22, 23, 4095, 4096}) {
                const int64_t c = host::stage_chunk_points(n, pairs);
                CHECK(c >= 1 && c <= n && (c % 1024 == 0 || c == n), "stage_chunk_points(%" PRId64 ", %" PRId64 ") = %" PRId64, n, pairs, c);
                CHECK(c * pairs * 16 <= host::RES_CHUNK_BYTES, "chunk of %" PRId64 " points x %" PRId64 " pairs passes the staging limit", c, pairs);
            }
            // normal_batch_grid: per pose the stripes cover every group exactly once and no workgroup is empty; blocks x B stays
            // below the aim + B -- for one pose: at most NORMAL_WG_PER_CU per CU and NORMAL_MAX_BLOCKS -- so the partial rows, 300
            // doubles each, stay bounded up to NORMAL_BATCH_MAX poses
            const int64_t aim = std::min<int64_t>((int64_t)cu * host::NORMAL_WG_PER_CU, host::NORMAL_MAX_BLOCKS);
            for (int64_t B : {1, 2, 3, 7, 64, 255, 256, 1000, 1023, 1024}) {
                const host::NormalGrid bg = host::normal_batch_grid(n, B, cu);
                CHECK(bg.blocks >= 1 && bg.groups_per >= 1 && (int64_t)bg.blocks * bg.groups_per >= rows &&
                          (int64_t)(bg.blocks - 1) * bg.groups_per < rows,
                      "normal_batch_grid(%" PRId64 ", %" PRId64 ", %d) = %d x %" PRId64 " does not tile %" PRId64 " groups", n, B, cu, bg.blocks,
                      bg.groups_per, rows);
                CHECK((int64_t)bg.blocks * B < aim + B && (int64_t)bg.blocks * B * 300 * 8 <= (int64_t)(host::NORMAL_MAX_BLOCKS + host::NORMAL_BATCH_MAX) * 300 * 8,
                      "normal_batch_grid(%" PRId64 ", %" PRId64 ", %d): %d x %" PRId64 " partial rows", n, B, cu, bg.blocks, B);
                int64_t bcovered = 0;
                for (int b = 0; b < bg.blocks; ++b) {        // the kernel's own stripe arithmetic: whole groups of 256 points
                    const int64_t beg = (int64_t)b * bg.groups_per * 256, end = std::min<int64_t>(beg + bg.groups_per * 256, n);
                    CHECK(beg == bcovered && end > beg && beg % 256 == 0 && (end % 256 == 0 || end == n),
                          "normal_batch_grid(%" PRId64 ", %" PRId64 ", %d): stripe %d is [%" PRId64 ", %" PRId64 ")", n, B, cu, b, beg, end);
                    bcovered = end;
                }
                CHECK(bcovered == n, "normal_batch_grid(%" PRId64 ", %" PRId64 ", %d) covers %" PRId64 " points", n, B, cu, bcovered);
            }
        }
    for (auto &nb : {std::pair<int64_t, int64_t>{0, 1}, {0, 64}, {1127, 0}, {1127, -1}, {0, 0}}) {
        const host::NormalGrid g = host::normal_batch_grid(nb.first, nb.second, 256);
        CHECK(g.blocks == 0 && g.groups_per == 0, "normal_batch_grid(%" PRId64 ", %" PRId64 ") launches %d workgroups", nb.first, nb.second, g.blocks);
    }
}

// ------------------------------------------------------------------ the render frame's plan (host/alp_plan.h)
// launch shapes over grids from one cell to 20000 x 20000 (sides around the 2^16-th vertex for the tile edge), frames from one
// pixel to the ABI's 32768 x 32768, small and large GPUs; then the overflow verdict: what grows exceeds what was asked for, what
// did not overflow keeps its capacity, and the verdict on the grown queues is "none" -- the reason finish_frame's loop ends
void check_frame_plan() {
    const int TW = 64, TH = 16;               // GT_W x GT_H of raster_plan.h
    const int64_t sides[] = {2, 3, 16, 17, 18, 64, 65, 66, 129, 1000, 3163, 10000, 20000, 65536, 65537, 65538};
    const int frames[][2] = {{1, 1}, {1, 255}, {16, 16}, {17, 15}, {320, 200}, {640, 427}, {5616, 3744}, {32768, 1}, {32768, 32768}};
    for (int cu : {1, 64, 256, 304})
        for (int64_t gh : sides)
            for (int64_t gw : sides) {
                if (gh * gw >= ((int64_t)1 << 31)) continue;                    // alp_mesh_create: fewer than 2^31 vertices
                for (auto &f : frames) {
                    const host::FramePlan p = host::frame_plan(true, gh, gw, 2 * (gh - 1) * (gw - 1), f[0], f[1], cu, TW, TH);
                    const int64_t tiles_y = p.tiles_x ? p.tiles / p.tiles_x : 0;
                    CHECK(p.tiles_x >= 1 && tiles_y >= 1 && p.tiles == p.tiles_x * tiles_y, "tiles of %" PRId64 " x %" PRId64, gh, gw);
                    CHECK((int64_t)p.tiles_x * TW >= gw - 1 && (int64_t)(p.tiles_x - 1) * TW < gw - 1 && tiles_y * TH >= gh - 1 &&
                              (tiles_y - 1) * TH < gh - 1, "the tiles of %" PRId64 " x %" PRId64 " do not cover its cells exactly", gh, gw);
                    CHECK(p.grid_wgs % 8 == 0 && p.grid_wgs >= p.tiles && p.grid_wgs < p.tiles + 8, "grid kernel: %u workgroups for %" PRId64 " tiles",
                          p.grid_wgs, p.tiles);
                    CHECK((int64_t)p.plan_grid * 256 >= p.tiles && ((int64_t)p.plan_grid - 1) * 256 < p.tiles, "plan grid %u for %" PRId64 " tiles",
                          p.plan_grid, p.tiles);
                    CHECK(p.tile_bounds_bytes == p.tiles * 24 && p.tile_lists_bytes == p.tiles * 12, "tile plan sizes");
                    CHECK(p.parked_wgs[0] == 8 * cu && p.parked_wgs[1] == 2 * cu && p.general_wgs == 2 * cu && p.large_wgs == 8 * cu && p.index_grid == 0,
                          "persistent grids at %d CUs", cu);
                    const int64_t blocks = ((int64_t)f[0] * f[1] + 255) / 256;
                    CHECK(p.resolve_grid >= 1 && p.resolve_grid <= 64 * cu && p.resolve_grid == std::min<int64_t>(blocks, 64 * cu),
                          "resolve grid %d for %d x %d at %d CUs", p.resolve_grid, f[0], f[1], cu);
                }
            }
    for (int cu : {1, 64, 256, 304})
        for (int64_t n_tri : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)64 * 256 * cu - 1, (int64_t)64 * 256 * cu,
                              (int64_t)64 * 256 * cu + 1, (int64_t)199960002, ((int64_t)1 << 32) - 2}) {
            const host::FramePlan p = host::frame_plan(false, 0, 0, n_tri, 1, 1, cu, TW, TH);
            CHECK(p.index_grid >= 1 && p.index_grid <= 64 * cu && p.index_grid == std::min<int64_t>((n_tri + 255) / 256, 64 * cu) && p.tiles == 0 &&
                      p.grid_wgs == 0 && p.resolve_grid == 1, "index grid %d for %" PRId64 " triangles at %d CUs", p.index_grid, n_tri, cu);
            // the tunables: other caps for the two capped grids only
            const host::FramePlan q = host::frame_plan(false, 0, 0, n_tri, 5616, 3744, cu, TW, TH, 16, 8);
            CHECK(q.index_grid == std::min<int64_t>((n_tri + 255) / 256, 16 * cu) && q.resolve_grid == std::min<int64_t>(82134, 8 * cu), "tunable caps");
        }
    // the start capacities
    CHECK(host::initial_queue_cap(nullptr) == (1u << 20) && host::initial_queue_cap("8") == 8 && host::initial_queue_cap("0") == (1u << 20) &&
              host::initial_queue_cap("-3") == (1u << 20) && host::initial_queue_cap("1073741824") == (1u << 20) &&
              host::initial_queue_cap("1073741823") == 1073741823u && host::initial_queue_cap("x") == (1u << 20), "ALP_QUEUE_CAP");
    for (unsigned cap : {1u, 8u, 1000u, 1u << 20, (1u << 20) + 1, (1u << 30) - 1}) {
        host::FrameQueues q;
        host::initial_park_caps(cap, &q);
        CHECK(q.park[0] == cap && q.park[1] == cap && q.park[2] == (cap == (1u << 20) ? 2u << 20 : cap), "parked queues of a start at %u", cap);
        for (int k = 0; k < 3; ++k) CHECK(q.park_b[k] == q.park[k] / 8 + 64, "second round of a start at %u", cap);
    }
    // the overflow verdict
    std::mt19937_64 rng(6);
    const unsigned levels[] = {0, 1, 7, 8, 9, 72, 1000, 1u << 20, (1u << 20) + 1, 3000000, 1u << 31};
    auto pick = [&] { return levels[rng() % (sizeof(levels) / sizeof(levels[0]))]; };
    for (int trial = 0; trial < 20000; ++trial) {
        const int stride = 8;
        unsigned c[16];
        for (unsigned &x : c) x = pick();
        host::FrameQueues have;
        have.items = std::max(pick(), 1u);
        have.general = std::max(pick(), 1u);
        const bool has_park = trial % 4 != 0;
        if (has_park) {
            host::FrameQueues start;
            host::initial_park_caps(std::max(pick(), 1u), &start);
            for (int k = 0; k < 3; ++k) {
                have.park[k] = trial % 3 ? start.park[k] : std::max(pick(), 1u);
                have.park_b[k] = trial % 3 ? start.park_b[k] : std::max(pick(), 1u);
            }
        }
        const host::QueueVerdict v = host::frame_verdict(c, stride, has_park, have);
        const unsigned items = std::max(c[0], c[stride]), general = std::max(c[1], c[stride + 1]);
        CHECK(v.items == (items > have.items) && v.general == (general > have.general), "work items / general entries: which overflowed");
        CHECK(v.items ? v.caps.items > items : v.caps.items == have.items, "work items %u of %u -> %u", items, have.items, v.caps.items);
        CHECK(v.general ? v.caps.general > general : v.caps.general == have.general, "general entries %u of %u -> %u", general, have.general, v.caps.general);
        bool park_over = false;
        for (int k = 0; k < 3; ++k) {
            const unsigned a = c[2 + k], b = c[stride + 2 + k];
            park_over |= has_park && (a > have.park[k] || b > have.park_b[k]);
            if (!has_park) {
                CHECK(v.caps.park[k] == have.park[k] && v.caps.park_b[k] == have.park_b[k], "parked counters count although no parked queues exist");
                continue;
            }
            CHECK(a > have.park[k] ? v.caps.park[k] > a : v.caps.park[k] == have.park[k], "first round, kind %d: %u of %u -> %u", k, a, have.park[k],
                  v.caps.park[k]);
            CHECK(v.caps.park_b[k] >= have.park_b[k] && v.caps.park_b[k] >= b, "second round, kind %d: %u of %u -> %u", k, b, have.park_b[k], v.caps.park_b[k]);
            CHECK(!v.park || v.caps.park_b[k] >= v.caps.park[k] / 8 + 64, "second round, kind %d, below an eighth of the first", k);
        }
        CHECK(v.park == park_over, "parked queues: which overflowed");
        if (!v.park)
            for (int k = 0; k < 3; ++k) CHECK(v.caps.park_b[k] == have.park_b[k], "second round changed without an overflow");
        CHECK(v.none() == !(v.items || v.general || v.park), "none()");
        const host::QueueVerdict again = host::frame_verdict(c, stride, has_park, v.caps);
        CHECK(again.none(), "the verdict on the grown queues is not none");
        CHECK(again.caps.items == v.caps.items && again.caps.general == v.caps.general, "none changes a capacity");
        for (int k = 0; k < 3; ++k) CHECK(again.caps.park[k] == v.caps.park[k] && again.caps.park_b[k] == v.caps.park_b[k], "none changes a capacity");
    }
}

// RowDiv::div(e) == e / w for every row length the grid form accepts (w <= 2^16) at the indices where a magic-number division
// fails first: around the multiples of w, spread over [0, 2^31), and at the top of the range
void check_row_div() {
    for (uint32_t w = 2; w <= 65536; ++w) {
        const RowDiv rd = host::row_div(w);
        const uint64_t mul = (((uint64_t)1 << rd.shift) + w - 1) / w;
        if (rd.w != w || mul > 0xffffffffull || rd.mul != (uint32_t)mul) CHECK(false, "row_div(%u): mul does not fit 32 bits", w);
        const uint32_t top = 0x7fffffffu, kmax = top / w;
        bool ok = true;
        for (uint32_t e : {0u, 1u, w - 1, w, w + 1, top, top - w + 1, kmax * w, kmax * w - 1}) ok &= rd.div(e) == e / w;
        for (uint32_t k = 1; k <= kmax; k += 1 + k / 3 + (w & 7)) {          // ~40 multiples, other ones for other w
            ok &= rd.div(k * w) == k && rd.div(k * w - 1) == k - 1;
        }
        if (!ok) CHECK(false, "RowDiv::div is not e / %u somewhere below 2^31", w);
    }
}

// RowWalk<VEC> against a division per point.  One vector of a set of n points in rows of w: a point that exists has the column
// and the row start its flat index gives; padding past the last point reads inside the column table and inside the y plane;
// one_row says exactly that the whole vector lies in e0's row.  Returns the number of vectors that were NOT one_row.
template <int VEC>
uint32_t row_walk_vector(const RowDiv &rd, uint32_t e0, uint32_t last) {
    const uint32_t w = rd.w;
    const RowWalk<VEC> walk(rd, e0, last);
    bool ok = walk.one_row == (e0 % w + VEC <= w);
    for (uint32_t k = 0; k < (uint32_t)VEC; ++k) {
        uint32_t col = ~0u, row0 = ~0u;
        walk.at(k, &col, &row0);
        const uint32_t e = std::min(e0 + k, last);
        if (e0 + k <= last || !walk.one_row) ok &= col == e % w && row0 == e / w * w;
        else ok &= col == e0 % w + k && row0 == e0 / w * w;       // padding of a one-row vector: the following columns
        ok &= col < w && row0 <= last;
    }
    if (!ok) CHECK(false, "RowWalk<%d>: w=%u e0=%u last=%u", VEC, w, e0, last);
    return walk.one_row ? 0 : 1;
}

template <int VEC>
void check_row_walk_t() {
    // every row length around the vector width with every point count up to a few rows (a grid set has n > w), every vector
    for (uint32_t w = 1; w <= 64; ++w) {
        const RowDiv rd = host::row_div(w);
        for (uint32_t n = w + 1; n <= 4 * w + VEC + 1; ++n) {
            uint32_t crossing = 0;
            for (uint32_t e0 = 0; e0 < n; e0 += VEC) crossing += row_walk_vector<VEC>(rd, e0, n - 1);
            if (w % VEC == 0) CHECK(crossing == 0, "RowWalk<%d>: w=%u n=%u leaves the one-row form", VEC, w, n);
        }
    }
    // random row lengths up to the cap with the set ending just below 2^31: the vectors around the last row ends and the last one
    std::mt19937_64 rng(VEC);
    for (int t = 0; t < 4000; ++t) {
        const uint32_t w = t < 8 ? 65536 - t : 1 + (uint32_t)(rng() % 65536);
        const RowDiv rd = host::row_div(w);
        const uint32_t n = 0x80000000u - (uint32_t)(rng() % (2 * w + 8));      // n_pad <= 2^31
        const uint32_t last = n - 1, rows = last / w;
        for (uint32_t r = rows >= 3 ? rows - 3 : 0; r <= rows; ++r)
            for (uint32_t e0 = (r * w - std::min(r * w, (uint32_t)(2 * VEC))) / VEC * VEC; e0 <= last && e0 < r * w + 2 * VEC; e0 += VEC)
                row_walk_vector<VEC>(rd, e0, last);
        for (uint32_t e0 = (last - std::min(last, (uint32_t)(3 * VEC))) / VEC * VEC; e0 <= last; e0 += VEC) row_walk_vector<VEC>(rd, e0, last);
        for (int s = 0; s < 16; ++s) row_walk_vector<VEC>(rd, (uint32_t)(rng() % n) / VEC * VEC, last);
    }
}

void check_row_walk() {
    check_row_walk_t<2>();
    check_row_walk_t<4>();
}

// ------------------------------------------------------------------ the launch plan of the descriptor matcher (host/alp_matchplan.h)
void check_match_plan() {
    // the padded length: the first instantiated K-step count that holds the descriptor, restated by counting up
    for (int len = 1; len <= MATCH_MAX_LEN; ++len) {
        const int ks = host::match_ksteps(len);
        int want = 0;
        for (int c = 1; c <= 16 && !want; ++c) {
            bool listed = false;
            for (int k : MATCH_KSTEPS) listed = listed || k == c;
            if (listed && c * MATCH_K >= len) want = c;
        }
        CHECK(ks == want && ks * MATCH_K >= len, "match_ksteps(%d) = %d, not %d", len, ks, want);
    }
    CHECK(host::match_ksteps(61) == 2 && host::match_ksteps(128) == 4 && host::match_ksteps(MATCH_MAX_LEN) == 16, "AKAZE / SIFT / longest");
    const int64_t edges[] = {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4096, 50000, 1000003};
    const int lens[] = {1, 31, 32, 33, 61, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 384, 385, 512};
    for (int len : lens)
        for (int esize : {1, 4})
            for (int cu : {1, 64, 256})
                for (int64_t nq : edges)
                    for (int64_t nt : edges) {
                        if (nt < 2) continue;
                        const int64_t tiles = (nt + 31) / 32;
                        for (int forced : {0, 1, 2, 3, (int)std::min<int64_t>(tiles, 1 << 20)}) {
                            const host::MatchPlan p = host::match_plan(nq, nt, len, esize, forced, cu);
                            CHECK(p.padded_len == p.ksteps * 32 && p.padded_len >= len && p.groups == (p.ksteps <= 4 ? 2 : 1) &&
                                      p.query_tile == 128 * p.groups && p.train_tile == 32,
                                  "tiles of len %d", len);
                            CHECK(p.train_tiles == tiles && p.nt_pad == tiles * 32 && p.nt_pad >= nt && p.nt_pad - nt < 32, "train tiles of %" PRId64, nt);
                            CHECK(p.nq_pad % p.query_tile == 0 && p.nq_pad >= nq && p.nq_pad - nq < p.query_tile && p.query_tiles * p.query_tile == p.nq_pad,
                                  "query tiles of %" PRId64, nq);
                            if (forced > tiles) continue;          // the entry point refuses it
                            if (forced) CHECK(p.splits == forced, "forced splits %d -> %d", forced, p.splits);
                            else {
                                // serial restatement: the first count that brings the grid to two workgroups per CU, capped by the tiles
                                int64_t s = 1;
                                while (s < tiles && s * p.query_tiles < 2 * cu) ++s;
                                if (p.query_tiles == 0) s = 1;
                                CHECK(p.splits == s, "splits(%" PRId64 " x %" PRId64 ", %d CUs) = %d, not %" PRId64, nq, nt, cu, p.splits, s);
                            }
                            CHECK(p.splits >= 1 && p.splits <= tiles && p.workgroups == p.query_tiles * p.splits, "grid");
                            // the splits cover the tiles once, in order, none empty
                            int64_t covered = 0;
                            for (int sp = 0; sp < p.splits; ++sp) {
                                int64_t b, e;
                                match_split_range(tiles, p.splits, sp, &b, &e);
                                CHECK(b == covered && e > b && e - b <= tiles / p.splits + 1, "split %d of %d over %" PRId64 " tiles: [%" PRId64 ", %" PRId64 ")",
                                      sp, p.splits, tiles, b, e);
                                covered = e;
                                if (p.splits > 64 && sp == 2) {     // (the long lists: both ends; the walk goes on at split splits - 3)
                                    sp = p.splits - 4;
                                    match_split_range(tiles, p.splits, sp + 1, &covered, &e);
                                }
                            }
                            CHECK(covered == tiles, "splits cover %" PRId64 " of %" PRId64 " tiles", covered, tiles);
                            // the device block: the arrays in order, aligned, none overlapping the next
                            const size_t off[] = {p.off_raw_q, p.off_raw_t, p.off_pack_q, p.off_pack_t, p.off_norm_q, p.off_norm_t, p.off_partial,
                                                  p.off_idx, p.off_dist2, p.off_dist, p.off_good, p.off_flags, p.scratch_bytes};
                            const size_t need[] = {(size_t)nq * len * esize, (size_t)nt * len * esize, (size_t)p.nq_pad * p.padded_len,
                                                   (size_t)p.nt_pad * p.padded_len, (size_t)p.nq_pad * 4, (size_t)p.nt_pad * 4,
                                                   (size_t)p.splits * p.nq_pad * 16, (size_t)nq * 8, (size_t)nq * 8, (size_t)nq * 8, (size_t)nq, 24};
                            CHECK(off[0] == 0, "first offset");
                            for (int i = 0; i < 12; ++i)
                                CHECK(off[i] % 256 == 0 && off[i + 1] >= off[i] + need[i] && off[i + 1] < off[i] + need[i] + 256 + 8, "array %d of the block", i);
                        }
                    }
    // the fragment order: a bijection of (row, byte) onto the packed array, 16 consecutive bytes of a row together
    for (int ks : MATCH_KSTEPS) {
        const int64_t rows = 96;
        std::vector<int> seen((size_t)rows * ks * 32, 0);
        for (int64_t r = 0; r < rows; ++r)
            for (int k = 0; k < ks * 32; ++k) {
                const size_t o = host::match_packed_offset(r, k, ks);
                CHECK(o < seen.size(), "packed offset of (%" PRId64 ", %d) outside the array", r, k);
                if (o < seen.size()) ++seen[o];
                if (k % 16) CHECK(o == host::match_packed_offset(r, k - 1, ks) + 1, "bytes %d and %d of a row apart", k - 1, k);
            }
        bool once = true;
        for (int v : seen) once = once && v == 1;
        CHECK(once, "fragment order with %d K steps is no bijection", ks);
    }
}

// ------------------------------------------------------------------ the launch plan of the geometric match filter (host/alp_epiplan.h)
void check_epi_plan() {
    // the caps: n in [8, 2^20], H in [1, 2^20], H * n <= 2^35, and nothing overflows on the way
    CHECK(!host::epi_caps_ok(7, 1) && host::epi_caps_ok(8, 1) && host::epi_caps_ok(EPI_MAX_N, 1) && !host::epi_caps_ok(EPI_MAX_N + 1, 1), "caps of n");
    CHECK(!host::epi_caps_ok(8, 0) && host::epi_caps_ok(8, EPI_MAX_H) && !host::epi_caps_ok(8, EPI_MAX_H + 1), "caps of H");
    CHECK(host::epi_caps_ok(1 << 15, EPI_MAX_H) && !host::epi_caps_ok((1 << 15) + 1, EPI_MAX_H) && !host::epi_caps_ok(EPI_MAX_N, EPI_MAX_H) &&
              host::epi_caps_ok(EPI_MAX_N, 1 << 15) && !host::epi_caps_ok(INT64_MAX, INT64_MAX) && !host::epi_caps_ok(-1, -1),
          "caps of H * n");
    // the essential filter: samples of 5, and a call of H samples is planned for 10 H slots, whose sample block (32 bytes a slot)
    // holds the H rows of 5 indices from byte 0 and the H solution counts from byte 32 H
    CHECK(!host::epi_caps_ok(4, 10, EPI_SAMPLE5) && host::epi_caps_ok(5, 10, EPI_SAMPLE5) && !host::epi_caps_ok(5, EPI_MAX_H + 10, EPI_SAMPLE5),
          "caps of the essential filter");
    for (int64_t H : {1, 26, 257, (int)(EPI_MAX_H / EPI_SLOTS5)}) {
        const host::EpiPlan p = host::epi_plan(5, H * EPI_SLOTS5, 0, 256);
        CHECK((size_t)H * EPI_SAMPLE5 * 4 <= (size_t)H * 32 && p.off_samples + (size_t)H * 36 <= p.off_F, "sample block of %" PRId64 " samples of 5", H);
        CHECK(p.off_F + (size_t)H * EPI_SLOTS5 * 72 <= p.off_partial && p.h_pad >= H * EPI_SLOTS5, "slots of %" PRId64 " samples of 5", H);
    }
    const int64_t ns[] = {8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 5000, 50000, 1 << 20};
    const int64_t hs[] = {1, 2, 63, 64, 65, 255, 256, 257, 1024, 16384, 131072, 600000, 1 << 20};
    for (int cu : {1, 64, 256})
        for (int64_t n : ns)
            for (int64_t H : hs) {
                if (!host::epi_caps_ok(n, H)) continue;
                const int64_t tiles = (n + EPI_MATCH_TILE - 1) / EPI_MATCH_TILE;
                for (int forced : {0, 1, 2, 3, 7, (int)tiles}) {
                    if (forced > tiles) continue;              // the entry point refuses it
                    const host::EpiPlan p = host::epi_plan(n, H, forced, cu);
                    CHECK(p.hyp_tile == 256 && p.match_tile == 512, "tiles");
                    CHECK(p.match_tiles == tiles && p.match_tiles * p.match_tile >= n && (p.match_tiles - 1) * p.match_tile < n, "match tiles of %" PRId64, n);
                    CHECK(p.h_pad == p.hyp_tiles * p.hyp_tile && p.h_pad >= H && p.h_pad - H < p.hyp_tile, "hypothesis tiles of %" PRId64, H);
                    CHECK(p.solve_blocks * EPI_SOLVE_BLOCK >= H && (p.solve_blocks - 1) * EPI_SOLVE_BLOCK < H, "solve blocks of %" PRId64, H);
                    CHECK(p.reduce_blocks >= 1 && p.reduce_blocks <= EPI_REDUCE_MAX_BLOCKS &&
                              (p.reduce_blocks == EPI_REDUCE_MAX_BLOCKS || (int64_t)p.reduce_blocks * EPI_REDUCE_BLOCK >= n),
                          "reduce blocks of %" PRId64, n);
                    if (forced) CHECK(p.splits == forced, "forced splits %d -> %d", forced, p.splits);
                    else {
                        // serial restatement: the first count that brings the grid to four workgroups per CU, capped by the tiles
                        int64_t s = 1;
                        while (s < tiles && s * p.hyp_tiles < 4 * cu) ++s;
                        CHECK(p.splits == s, "splits(%" PRId64 " x %" PRId64 ", %d CUs) = %d, not %" PRId64, n, H, cu, p.splits, s);
                    }
                    CHECK(p.splits >= 1 && p.splits <= tiles && p.workgroups == p.hyp_tiles * p.splits && p.workgroups < ((int64_t)1 << 31), "grid");
                    // the splits cover the match tiles once, in order, none empty
                    int64_t covered = 0;
                    for (int sp = 0; sp < p.splits; ++sp) {
                        int64_t b, e;
                        match_split_range(tiles, p.splits, sp, &b, &e);
                        CHECK(b == covered && e > b, "split %d of %d over %" PRId64 " tiles: [%" PRId64 ", %" PRId64 ")", sp, p.splits, tiles, b, e);
                        covered = e;
                    }
                    CHECK(covered == tiles, "splits cover %" PRId64 " of %" PRId64 " tiles", covered, tiles);
                    // the device block: the arrays in order, aligned, none overlapping the next
                    const size_t off[] = {p.off_raw1, p.off_raw2, p.off_pts, p.off_samples, p.off_F, p.off_partial, p.off_counts, p.off_state,
                                          p.off_sym, p.off_cpart, p.off_mask, p.off_err, p.scratch_bytes};
                    const size_t need[] = {(size_t)n * 16, (size_t)n * 16, (size_t)n * 32, (size_t)H * 32, (size_t)H * 72, (size_t)p.splits * p.h_pad * 4,
                                           (size_t)H * 4, (size_t)EPI_STATE_BYTES, (size_t)p.reduce_blocks * EPI_SYM * 8, (size_t)p.reduce_blocks * 4,
                                           (size_t)n, (size_t)n * 8};
                    CHECK(off[0] == 0, "first offset");
                    for (int i = 0; i < 12; ++i)
                        CHECK(off[i] % 256 == 0 && off[i + 1] >= off[i] + need[i] && off[i + 1] < off[i] + need[i] + 256, "array %d of the block", i);
                    CHECK(p.passes == 0 && p.hist_bytes == 0 && p.off_hist == 0 && p.off_prefix == 0 && p.off_rank == 0 && p.off_value == 0,
                          "the counting path plans no select");
                    // the plan of the LMedS select: the counting path's plan word for word, then its own arrays, aligned and disjoint
                    if (!host::epi_select_caps_ok(n, H)) continue;
                    const host::EpiPlan q = host::epi_select_plan(n, H, forced, cu);
                    CHECK(q.splits == p.splits && q.splits <= tiles && q.workgroups == p.workgroups && q.h_pad == p.h_pad && q.match_tiles == p.match_tiles &&
                              q.reduce_blocks == p.reduce_blocks && q.solve_blocks == p.solve_blocks,
                          "the select's launch plan is the score's");
                    const size_t qoff[] = {q.off_raw1, q.off_raw2, q.off_pts, q.off_samples, q.off_F, q.off_partial, q.off_counts, q.off_state,
                                           q.off_sym, q.off_cpart, q.off_mask, q.off_err};
                    for (int i = 0; i < 12; ++i) CHECK(qoff[i] == off[i], "offset %d moved under the select's plan", i);
                    CHECK(q.passes == EPI_SELECT_PASSES && q.passes * EPI_SELECT_BITS == 64 && (int64_t)q.passes * H <= EPI_MAX_WORK / n, "passes and their work");
                    CHECK(q.hist_bytes == (size_t)q.splits * EPI_SELECT_DIGITS * q.h_pad * 4, "bytes of the partial histograms");
                    const size_t soff[] = {p.scratch_bytes, q.off_hist, q.off_prefix, q.off_rank, q.off_value, q.scratch_bytes};
                    const size_t sneed[] = {0, q.hist_bytes, (size_t)q.h_pad * 8, (size_t)q.h_pad * 4, (size_t)H * 8};
                    CHECK(q.off_hist == p.scratch_bytes, "the select's arrays start where the counting path's block ends");
                    for (int i = 0; i < 5; ++i)
                        CHECK(soff[i] % 256 == 0 && soff[i + 1] >= soff[i] + sneed[i] && soff[i + 1] < soff[i] + sneed[i] + 256, "array %d of the select", i);
                }
            }
    // the caps of the select: 16 passes * H * n <= 2^35 on top of the others
    CHECK(host::epi_select_caps_ok(1 << 11, EPI_MAX_H) && !host::epi_select_caps_ok((1 << 11) + 1, EPI_MAX_H) && host::epi_select_caps_ok(EPI_MAX_N, 1 << 11) &&
              !host::epi_select_caps_ok(EPI_MAX_N, (1 << 11) + 1) && !host::epi_select_caps_ok(7, 1) && host::epi_select_caps_ok(5, 10, EPI_SAMPLE5) &&
              !host::epi_select_caps_ok(INT64_MAX, INT64_MAX) && !host::epi_select_caps_ok(-1, -1) && host::epi_select_caps_ok(5000, 163840, EPI_SAMPLE5),
          "caps of the select");
}

// ------------------------------------------------------------------ the error message is per thread
void check_errors() {
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
        th.emplace_back([t] {
            for (int k = 0; k < 2000; ++k) {
                const int code = fail(ALP_EINVAL, "thread %d call %d", t, k);
                char want[64];
                snprintf(want, sizeof(want), "thread %d call %d", t, k);
                CHECK(code == ALP_EINVAL && !strcmp(alp_last_error(), want), "message of another thread: %s", alp_last_error());
            }
        });
    for (auto &x : th) x.join();
}

}  // namespace

// Deliberate defects, one per sanitizer: tests/test_host_sanitized.py expects the matching build to REPORT them -- a
// sanitizer that says nothing about these says nothing by staying silent on the real code either.
int canary(const char *which) {
    if (!strcmp(which, "overflow")) {                           // AddressSanitizer: one float past a conversion's destination
        std::vector<float> src(70001, 1.0f);
        std::vector<double> dst(70000);
        host::convert_threads(src.data(), dst.data(), 70001, 4);
        return dst[69999] == 1.0 ? 0 : 1;
    }
    if (!strcmp(which, "race")) {                               // ThreadSanitizer: two workers given overlapping shares
        std::vector<float> src(1 << 17, 1.0f);
        std::vector<double> dst(1 << 17);
        std::atomic<int> gate{0};                               // both workers write at the same time, as the real ones do
        auto arrive = [&] { gate.fetch_add(1); while (gate.load() < 2) {} };
        std::thread a([&] { arrive(); host::convert_slice(src.data(), dst.data(), (int64_t)1 << 17); });
        std::thread b([&] { arrive(); host::convert_slice(src.data(), dst.data() + 16, ((int64_t)1 << 17) - 16); });
        a.join();
        b.join();
        return 0;
    }
    if (!strcmp(which, "shift")) {                              // UndefinedBehaviorSanitizer: a 64-bit rotate by 64
        volatile int r = 64;
        volatile uint64_t x = 1;
        return (int)((x << r) & 1);
    }
    return 2;
}

// --plan: one query per argument, or per line of stdin when there is none: n,P,f32|f64,V,TC,cu,batched,pairs[,stripes,tile_cols]
// (the last two: an ALP_POP_GRID pair) -> "stripes tile_cols chunk_points stream_grid confirm_grid";
// normal,n,cu -> "blocks groups_per" of normal_batch_grid for one pose
// normal_batch,n,B,cu -> "blocks groups_per" of normal_batch_grid (blocks = the stripes per pose), 1 <= B <= NORMAL_BATCH_MAX
// mend,n,P,V,TC,cu -> "stripes tile_cols" of mend_grid
// epi,n,H,forced_splits,cu -> "hyp_tile match_tile splits hyp_tiles match_tiles workgroups solve_blocks reduce_blocks bytes" of epi_plan
// lmeds,n,H,forced_splits,cu -> the same of epi_select_plan, then "passes hist_bytes off_hist off_prefix off_rank off_value"
// frame,implicit,grid_h,grid_w,n_tri,w,h,cu,tile_w,tile_h -> "tiles_x tiles plan_grid grid_wgs parked_wgs[0] parked_wgs[1] general_wgs large_wgs
//   index_grid resolve_grid tile_bounds_bytes tile_lists_bytes" of frame_plan
// queues,ALP_QUEUE_CAP text or '-' -> "cap small large cells small_b large_b cells_b": the start capacities
// verdict,has_park,items,general,small,large,cells,small_b,large_b,cells_b,<10 counters: [0] .. [4] of round 0, then of round 1>
//   -> "items|-  general|-  park|-" then the eight capacities in the order given: what must be allocated anew, and how large
int frame_query(const char *q) {
    if (!strncmp(q, "frame,", 6)) {
        int implicit = 0, w = 0, h = 0, cu = 0, tw = 0, th = 0;
        long long gh = 0, gw = 0, n_tri = 0;
        if (sscanf(q + 6, "%d,%lld,%lld,%lld,%d,%d,%d,%d,%d", &implicit, &gh, &gw, &n_tri, &w, &h, &cu, &tw, &th) != 9 || w < 1 || h < 1 || cu < 1 ||
            tw < 1 || th < 1)
            return 2;
        const host::FramePlan p = host::frame_plan(implicit != 0, gh, gw, n_tri, w, h, cu, tw, th);
        printf("%d %lld %u %u %d %d %d %d %d %d %lld %lld\n", p.tiles_x, (long long)p.tiles, p.plan_grid, p.grid_wgs, p.parked_wgs[0], p.parked_wgs[1],
               p.general_wgs, p.large_wgs, p.index_grid, p.resolve_grid, (long long)p.tile_bounds_bytes, (long long)p.tile_lists_bytes);
        return 0;
    }
    if (!strncmp(q, "queues,", 7)) {
        char text[32] = "";
        if (sscanf(q + 7, "%31[^,\n]", text) != 1) return 2;
        host::FrameQueues fq;
        const unsigned cap = host::initial_queue_cap(strcmp(text, "-") ? text : nullptr);
        host::initial_park_caps(cap, &fq);
        printf("%u %u %u %u %u %u %u\n", cap, fq.park[0], fq.park[1], fq.park[2], fq.park_b[0], fq.park_b[1], fq.park_b[2]);
        return 0;
    }
    int has_park = 0;
    unsigned c[16] = {0}, *r1 = c + 8;
    host::FrameQueues have;
    if (sscanf(q, "verdict,%d,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u", &has_park, &have.items, &have.general, &have.park[0], &have.park[1],
               &have.park[2], &have.park_b[0], &have.park_b[1], &have.park_b[2], c, c + 1, c + 2, c + 3, c + 4, r1, r1 + 1, r1 + 2, r1 + 3, r1 + 4) != 19)
        return 2;
    const host::QueueVerdict v = host::frame_verdict(c, 8, has_park != 0, have);
    printf("%s %s %s %u %u %u %u %u %u %u %u\n", v.items ? "items" : "-", v.general ? "general" : "-", v.park ? "park" : "-", v.caps.items, v.caps.general,
           v.caps.park[0], v.caps.park[1], v.caps.park[2], v.caps.park_b[0], v.caps.park_b[1], v.caps.park_b[2]);
    return 0;
}

int plan_query(const char *q) {
    if (!strncmp(q, "frame,", 6) || !strncmp(q, "queues,", 7) || !strncmp(q, "verdict,", 8)) {
        const int rc = frame_query(q);
        if (rc) fprintf(stderr, "bad plan query: %s\n", q);
        return rc;
    }
    if (!strncmp(q, "normal_batch,", 13)) {
        long long nn = -1, nb = 0;
        int ncu = 0;
        if (sscanf(q + 13, "%lld,%lld,%d", &nn, &nb, &ncu) != 3 || nn < 0 || nb < 1 || nb > host::NORMAL_BATCH_MAX || ncu < 1) {
            fprintf(stderr, "bad plan query: %s\n", q);
            return 2;
        }
        const host::NormalGrid g = host::normal_batch_grid(nn, nb, ncu);
        printf("%d %lld\n", g.blocks, (long long)g.groups_per);
        return 0;
    }
    if (!strncmp(q, "normal,", 7)) {
        long long nn = -1;
        int ncu = 0;
        if (sscanf(q + 7, "%lld,%d", &nn, &ncu) != 2 || nn < 0 || ncu < 1) {
            fprintf(stderr, "bad plan query: %s\n", q);
            return 2;
        }
        const host::NormalGrid g = host::normal_batch_grid(nn, 1, ncu);
        printf("%d %lld\n", g.blocks, (long long)g.groups_per);
        return 0;
    }
    if (!strncmp(q, "epi,", 4)) {
        long long nn = 0, hh = 0;
        int forced = 0, ecu = 0;
        if (sscanf(q + 4, "%lld,%lld,%d,%d", &nn, &hh, &forced, &ecu) != 4 || !host::epi_caps_ok(nn, hh) || forced < 0 || ecu < 1 ||
            forced > (nn + EPI_MATCH_TILE - 1) / EPI_MATCH_TILE) {
            fprintf(stderr, "bad plan query: %s\n", q);
            return 2;
        }
        const host::EpiPlan p = host::epi_plan(nn, hh, forced, ecu);
        printf("%d %d %d %lld %lld %lld %lld %d %lld\n", p.hyp_tile, p.match_tile, p.splits, (long long)p.hyp_tiles, (long long)p.match_tiles,
               (long long)p.workgroups, (long long)p.solve_blocks, p.reduce_blocks, (long long)p.scratch_bytes);
        return 0;
    }
    if (!strncmp(q, "lmeds,", 6)) {
        long long nn = 0, hh = 0;
        int forced = 0, ecu = 0;
        if (sscanf(q + 6, "%lld,%lld,%d,%d", &nn, &hh, &forced, &ecu) != 4 || !host::epi_select_caps_ok(nn, hh) || forced < 0 || ecu < 1 ||
            forced > (nn + EPI_MATCH_TILE - 1) / EPI_MATCH_TILE) {
            fprintf(stderr, "bad plan query: %s\n", q);
            return 2;
        }
        const host::EpiPlan p = host::epi_select_plan(nn, hh, forced, ecu);
        printf("%d %d %d %lld %lld %lld %lld %d %lld %d %lld %lld %lld %lld %lld\n", p.hyp_tile, p.match_tile, p.splits, (long long)p.hyp_tiles,
               (long long)p.match_tiles, (long long)p.workgroups, (long long)p.solve_blocks, p.reduce_blocks, (long long)p.scratch_bytes, p.passes,
               (long long)p.hist_bytes, (long long)p.off_hist, (long long)p.off_prefix, (long long)p.off_rank, (long long)p.off_value);
        return 0;
    }
    if (!strncmp(q, "mend,", 5)) {
        long long nn = -1, PP = 0;
        int mV = 0, mTC = 0, mcu = 0;
        if (sscanf(q + 5, "%lld,%lld,%d,%d,%d", &nn, &PP, &mV, &mTC, &mcu) != 5 || nn < 0 || PP < 1 || mV < 1 || mTC < 1 || mcu < 1) {
            fprintf(stderr, "bad plan query: %s\n", q);
            return 2;
        }
        const host::PopGrid g = host::mend_grid(nn, PP, mV, mTC, mcu);
        printf("%d %d\n", g.stripes, g.tile_cols);
        return 0;
    }
    long long n = 0, P = 0, pairs = 0;
    char prec[4] = "";
    int V = 0, TC = 0, cu = 0, batched = 0, a = 0, b = 0;
    const int got = sscanf(q, "%lld,%lld,%3[f0-9],%d,%d,%d,%d,%lld,%d,%d", &n, &P, prec, &V, &TC, &cu, &batched, &pairs, &a, &b);
    const bool f64 = !strcmp(prec, "f64");
    if ((got != 8 && got != 10) || (!f64 && strcmp(prec, "f32")) || n < 0 || P < 1 || V < 1 || TC < 1 || cu < 1 || pairs < 1) {
        fprintf(stderr, "bad plan query: %s\n", q);
        return 2;
    }
    const host::PopGrid g = host::pop_grid(n, P, f64, V, TC, cu, batched != 0, a, b);
    printf("%d %d %lld %d %d\n", g.stripes, g.tile_cols, (long long)host::stage_chunk_points(n, pairs), host::stream_grid(n, cu),
           host::confirm_grid(n, cu));
    return 0;
}

int plan(int argc, char **argv) {
    for (int i = 0; i < argc; ++i)
        if (int rc = plan_query(argv[i])) return rc;
    char line[256];
    while (argc == 0 && fgets(line, sizeof(line), stdin))
        if (int rc = line[0] == '\n' ? 0 : plan_query(line)) return rc;
    return 0;
}

// ------------------------------------------------------------------ the Levenberg-Marquardt state machine (host/alp_lm.h)
// cost = 0.5 |A x - b|^2 of a small built-in problem: G = A^T A and g = A^T (A x - b) are exact, so the machine must reach the
// least-squares solution (unbounded) or the box-constrained one (a bound active), and every stop must be one of its own.
struct LmQuadratic {
    static constexpr int M = 6, D = 3;
    double A[M][D], b[M];
    LmQuadratic() {
        const double a[M][D] = {{4, 1, 0}, {1, 3, 1}, {0, 1, 50}, {2, 0, 1}, {1, 1, 1}, {0, 2, 3}};
        const double want[D] = {0.5, -0.25, 0.75};
        for (int i = 0; i < M; ++i) {
            b[i] = 0;
            for (int j = 0; j < D; ++j) { A[i][j] = a[i][j]; b[i] += a[i][j] * want[j]; }
        }
    }
    double sums(const double *x, double *G, double *g) const {
        double r[M], cost = 0;
        for (int i = 0; i < M; ++i) {
            r[i] = -b[i];
            for (int j = 0; j < D; ++j) r[i] += A[i][j] * x[j];
            cost += 0.5 * r[i] * r[i];
        }
        int t = 0;
        for (int i = 0; i < D; ++i)
            for (int j = i; j < D; ++j, ++t) {
                G[t] = 0;
                for (int k = 0; k < M; ++k) G[t] += A[k][i] * A[k][j];
            }
        for (int j = 0; j < D; ++j) {
            g[j] = 0;
            for (int k = 0; k < M; ++k) g[j] += A[k][j] * r[k];
        }
        return cost;
    }
};

void lm_run(const LmConfig &cfg, const LmQuadratic &q, const double *x0, LmState *s, const double *first_cost = nullptr) {
    double work[LM_WORK], G[LM_TRI], g[LM_MAX_D];
    lm_start(cfg, x0, s);
    for (int round = 0; s->phase != LM_STOPPED && round < 10000; ++round) {
        double cost = q.sums(s->trial, G, g);
        if (round == 0 && first_cost) cost = *first_cost;
        lm_advance(cfg, s, G, g, cost, work);
    }
}

void check_lm() {
    const LmQuadratic q;
    LmConfig cfg{};
    cfg.D = 3;
    cfg.ftol = cfg.xtol = cfg.gtol = 1e-10;
    cfg.max_nfev = 300;
    const double x0[3] = {-0.9, 0.9, -0.9}, want[3] = {0.5, -0.25, 0.75};
    LmState s;
    for (int i = 0; i < 3; ++i) { cfg.lower[i] = -INFINITY; cfg.upper[i] = INFINITY; }
    lm_run(cfg, q, x0, &s);
    CHECK(s.status >= 1 && s.status <= 4 && s.phase == LM_STOPPED, "unbounded: status %d", s.status);
    for (int i = 0; i < 3; ++i) CHECK(std::fabs(s.x[i] - want[i]) < 1e-7, "unbounded: x[%d] = %.17g", i, s.x[i]);
    CHECK(s.nfev >= 2 && s.nfev <= 300 && s.iterations >= 1 && s.iterations < s.nfev, "unbounded: %d evaluations, %d iterations", s.nfev, s.iterations);
    // a box whose upper bound cuts x[2] off: the optimum lies on it, and the gradient there pushes outward
    for (int i = 0; i < 3; ++i) { cfg.lower[i] = -1; cfg.upper[i] = 1; }
    cfg.upper[2] = 0.5;
    lm_run(cfg, q, x0, &s);
    CHECK(s.status >= 1 && s.status <= 4, "bounded: status %d", s.status);
    CHECK(s.x[2] == 0.5 && s.g[2] < 0 && lm_grad_norm(cfg, &s) < 1e-4, "bounded: x[2] = %.17g, g[2] = %g, |g| free = %g", s.x[2], s.g[2],
          lm_grad_norm(cfg, &s));
    for (int i = 0; i < 3; ++i) CHECK(s.x[i] >= cfg.lower[i] && s.x[i] <= cfg.upper[i], "bounded: x[%d] outside the box", i);
    // the stops that need no solve: a cost that is not finite at x0, max_nfev = 1, every variable on a bound it is pushed against
    const double nan = NAN;
    lm_run(cfg, q, x0, &s, &nan);
    CHECK(s.status == -1 && s.nfev == 1 && s.iterations == 0 && lm_grad_norm(cfg, &s) != lm_grad_norm(cfg, &s), "NaN at x0: status %d", s.status);
    cfg.max_nfev = 1;
    lm_run(cfg, q, x0, &s);
    CHECK(s.status == 0 && s.nfev == 1, "max_nfev = 1: status %d after %d", s.status, s.nfev);
    cfg.max_nfev = 300;
    for (int i = 0; i < 3; ++i) { cfg.lower[i] = 2; cfg.upper[i] = 3; }
    lm_run(cfg, q, x0, &s);
    CHECK(s.status == 1 && s.nfev == 1 && s.x[0] == 2 && s.x[1] == 2 && s.x[2] == 2, "all on bounds: status %d after %d", s.status, s.nfev);
}

// --lm: the machine on sums read from stdin.  "D max_nfev ftol xtol gtol", then x0, lower and upper (D numbers each; inf and
// hexadecimal floats are read), then rows of D (D + 1) / 2 + D + 1 numbers: G (row-major upper triangle), g and the cost at the
// pending trial point.  Prints "trial <D numbers>" for every trial point (the first one before any row is read) and, when the
// machine stops or the rows run out, "final status evaluations iterations cost grad_norm mu nu <x>" ("starved" instead of
// "final" when it had not stopped).  Numbers are printed as %a.
int lm_mode() {
    LmConfig cfg{};
    int D = 0, max_nfev = 0;
    if (scanf("%d %d %lf %lf %lf", &D, &max_nfev, &cfg.ftol, &cfg.xtol, &cfg.gtol) != 5 || D < 1 || D > LM_MAX_D || max_nfev < 1) {
        fprintf(stderr, "bad --lm header\n");
        return 2;
    }
    cfg.D = D;
    cfg.max_nfev = max_nfev;
    double x0[LM_MAX_D], row[LM_TRI + LM_MAX_D + 1], work[LM_WORK];
    for (double *dst : {x0, cfg.lower, cfg.upper})
        for (int i = 0; i < D; ++i)
            if (scanf("%lf", dst + i) != 1) {
                fprintf(stderr, "bad --lm start or bounds\n");
                return 2;
            }
    const int tri = D * (D + 1) / 2, T = tri + D + 1;
    LmState s;
    lm_start(cfg, x0, &s);
    auto trial = [&] {
        printf("trial");
        for (int i = 0; i < D; ++i) printf(" %a", s.trial[i]);
        printf("\n");
    };
    trial();
    while (s.phase != LM_STOPPED) {
        int got = 0;
        while (got < T && scanf("%lf", row + got) == 1) ++got;
        if (got == 0) break;
        if (got != T) {
            fprintf(stderr, "bad --lm row: %d of %d numbers\n", got, T);
            return 2;
        }
        lm_advance(cfg, &s, row, row + tri, row[T - 1], work);
        if (s.phase != LM_STOPPED) trial();
    }
    printf("%s %d %d %d %a %a %a %a", s.phase == LM_STOPPED ? "final" : "starved", s.status, s.nfev, s.iterations, s.cost, lm_grad_norm(cfg, &s),
           s.mu, s.nu);
    for (int i = 0; i < D; ++i) printf(" %a", s.x[i]);
    printf("\n");
    return 0;
}

// ------------------------------------------------------------------ Buffer / reserve_all (host/alp_buffer.h)
// The memory policy of this group: malloc and free (so a leak, a double free or a use after release is the sanitizers' to
// report), counted, and told to fail the k-th allocation from now.  Only this group's thread touches it.
struct CountedMemory {
    static int live, peak, allocs, fail_at;      // blocks held now / at most since `peak` was reset; calls; the call to fail (0: none)
    static int alloc(void **p, size_t bytes) {
        if (++allocs == fail_at) return fail(ALP_EHIP, "counted allocation %d failed", allocs);
        *p = malloc(bytes ? bytes : 1);
        memset(*p, 0xA5, bytes);
        ++live;
        peak = std::max(peak, live);
        return ALP_OK;
    }
    static void release(void *p) {
        free(p);
        --live;
    }
    static void fail_next(int k) { allocs = 0, fail_at = k; }
};
int CountedMemory::live = 0, CountedMemory::peak = 0, CountedMemory::allocs = 0, CountedMemory::fail_at = 0;

void check_buffer() {
    using Mem = CountedMemory;
    using Bytes = Buffer<Mem, unsigned char>;
    {
        Bytes b;
        CHECK(!b && b.get() == nullptr && b.capacity() == 0 && Mem::live == 0, "a new buffer is not empty");
        CHECK(b.reserve(100) == ALP_OK && b && b.capacity() == 100 && Mem::live == 1, "first reserve");
        unsigned char *first = b;
        b[99] = 7;
        // a reserve that fits keeps the block (and what is in it)
        CHECK(b.reserve(100) == ALP_OK && b.reserve(1) == ALP_OK && b.get() == first && b.capacity() == 100 && b[99] == 7,
              "a reserve that fits moved the block");
        CHECK(Mem::live == 1, "a reserve that fits left %d blocks", Mem::live);
        // a reserve that grows releases first: never more blocks live than before the call
        Mem::peak = Mem::live;
        CHECK(b.reserve(101) == ALP_OK && b.capacity() == 101 && Mem::live == 1 && Mem::peak == 1,
              "growing held %d blocks at once", Mem::peak);
        b[100] = 1;
        // a failed reserve: empty, capacity 0, nothing live, the policy's code
        Mem::fail_next(1);
        CHECK(b.reserve(1000) == ALP_EHIP && !b && b.capacity() == 0 && Mem::live == 0,
              "a failed reserve left %d block(s)", Mem::live);
        CHECK(strstr(alp_last_error(), "counted allocation") != nullptr, "error text: %s", alp_last_error());
        Mem::fail_next(0);
        CHECK(b.reserve(8) == ALP_OK && b.capacity() == 8 && Mem::live == 1, "reserve after a failure");
        b.reset();
        CHECK(!b && b.capacity() == 0 && Mem::live == 0, "reset");
        b.reset();                                  // (of an empty buffer: nothing to release)
        CHECK(Mem::live == 0, "second reset");
    }
    {   // moves: the source comes out empty, a block the target held is released
        Bytes a;
        CHECK(a.reserve(16) == ALP_OK, "reserve");
        unsigned char *pa = a;
        Bytes b(std::move(a));
        CHECK(!a && a.capacity() == 0 && b.get() == pa && b.capacity() == 16 && Mem::live == 1, "move construction");
        Bytes c;
        c = std::move(b);
        CHECK(!b && c.get() == pa && c.capacity() == 16 && Mem::live == 1, "move assignment to an empty buffer");
        Bytes d;
        CHECK(d.reserve(32) == ALP_OK && Mem::live == 2, "reserve");
        d = std::move(c);
        CHECK(!c && d.get() == pa && d.capacity() == 16 && Mem::live == 1, "move assignment onto a block left %d live", Mem::live);
        Bytes &self = d;
        d = std::move(self);
        CHECK(d.get() == pa && Mem::live == 1, "self-assignment");
        Buffer<Mem> v;                              // the untyped form reads like a void *
        CHECK(v.reserve(8) == ALP_OK && (const float *)v == (const float *)v.get() && (char *)v + 4 == (char *)v.get() + 4, "casts");
    }
    CHECK(Mem::live == 0, "%d block(s) outlived their buffers", Mem::live);
    // groups of 2 and 3: whichever member fails, the whole group comes out empty -- the members that held a block before the
    // call included -- and the next call succeeds
    for (int size = 2; size <= 3; ++size)
        for (int bad = 1; bad <= size; ++bad)
            for (int held = 0; held < 2; ++held) {
                Buffer<Mem, double> x;
                Buffer<Mem> y;
                Buffer<Mem, int> z;
                auto group = [&](size_t n) {
                    return size == 2 ? reserve_all({n, 2 * n}, x, y) : reserve_all({n, 2 * n, 3 * n}, x, y, z);
                };
                if (held) CHECK(group(8) == ALP_OK && Mem::live == size, "first group");
                Mem::fail_next(bad);
                CHECK(group(64) == ALP_EHIP && !x && !y && !z && x.capacity() + y.capacity() + z.capacity() == 0 && Mem::live == 0,
                      "group of %d, member %d failed (held %d): %d block(s) live", size, bad, held, Mem::live);
                Mem::fail_next(0);
                CHECK(group(64) == ALP_OK && x && y && (size == 2 || z) && x.capacity() == 64 && y.capacity() == 128,
                      "group of %d after a failure", size);
                CHECK(Mem::live == size, "group of %d after a failure: %d blocks", size, Mem::live);
                x[7] = 1.0;                         // (the last element each: the sanitizers hold the sizes to it)
                ((char *)y)[127] = 1;
                if (size == 3) z[47] = 1;
                double *px = x;
                CHECK(group(64) == ALP_OK && x.get() == px && Mem::live == size, "a group that fits moved");
                reset_all(x, y, z);
                CHECK(Mem::live == 0, "reset_all");
            }
    CHECK(Mem::live == 0, "%d block(s) live at the end", Mem::live);
}

int main(int argc, char **argv) {
    if (argc > 2 && !strcmp(argv[1], "--canary")) return canary(argv[2]);
    if (argc > 1 && !strcmp(argv[1], "--plan")) return plan(argc - 2, argv + 2);
    if (argc > 1 && !strcmp(argv[1], "--lm")) return lm_mode();
    struct Group { const char *name; void (*fn)(); };
    const Group groups[] = {{"hash", check_hash},     {"minmax", check_minmax},   {"prefault", check_prefault}, {"fold_pose", check_fold_pose},
                            {"convert", check_convert}, {"grid", check_grid},     {"selection", check_selection}, {"errors", check_errors},
                            {"plan", check_plan},       {"frame_plan", check_frame_plan}, {"row_div", check_row_div}, {"lm", check_lm},
                            {"buffer", check_buffer},   {"row_walk", check_row_walk}, {"match_plan", check_match_plan},
                            {"epi_plan", check_epi_plan}};
    const bool concurrent = !(argc > 1 && !strcmp(argv[1], "--serial"));
    // every group on its own caller thread at once: the library promises that independent calls may overlap
    std::vector<std::thread> th;
    for (const Group &g : groups) {
        if (concurrent) th.emplace_back(g.fn);
        else g.fn();
    }
    for (auto &x : th) x.join();
    // ... and the same helper from two caller threads at once
    std::thread a(check_convert), b(check_convert);
    check_selection();
    a.join();
    b.join();
    if (g_failures.load()) {
        fprintf(stderr, "host selfcheck: %d comparison(s) failed\n", g_failures.load());
        return 1;
    }
    printf("host selfcheck ok: %zu groups%s\n", sizeof(groups) / sizeof(groups[0]), concurrent ? ", run concurrently" : "");
    return 0;
}
