// The candidate draw of the CMA-ES sampler, shared by alp_cma_sample (alp_sampler.hip) and the device loop of the generation
// (alp_cma.hip): the counter-based generator, the D normal deviates of one try and x = mean + sigma * BD z with its box test.
// Both translation units inline the same code, so that a candidate of the device loop is bit for bit the one
// alp_cma_sample draws for the same seed, generation, mean, sigma and BD.  Every multiply-add is written as fma() (the
// device loop is compiled with -ffp-contract=off).
#pragma once

#include "alp_internal.h"

#include <cmath>

namespace alp {

constexpr int SAMPLER_MAX_D = 32;

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// D standard normal deviates of (try, candidate, generation): Box-Muller on 53-bit uniforms
template <int DMAX>
__device__ __forceinline__ void draw_normals(double (&z)[DMAX], int D, unsigned tr, unsigned cand, unsigned gen, unsigned k0, unsigned k1) {
#pragma unroll
    for (int j = 0; j < DMAX; j += 2) {
        if (j < D) {                 // predicated, so that the loop unrolls and z[] lives in registers
            unsigned w[4];
            philox4x32_10((unsigned)(j >> 1), tr, cand, gen, k0, k1, w);
            const double u1 = ((double)(((unsigned long long)w[0] << 21) | (w[1] >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
            const double u2 = ((double)(((unsigned long long)w[2] << 21) | (w[3] >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
            const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586476925286766559 * u2;
            z[j] = rad * cos(ang);
            if (j + 1 < DMAX) z[j + 1] = (j + 1 < D) ? rad * sin(ang) : 0.0;
        }
    }
}

struct SamplerArgs {
    double mean[SAMPLER_MAX_D], lower[SAMPLER_MAX_D], upper[SAMPLER_MAX_D];
    double sigma;
    int D, n_max, bounded;
    unsigned k0, k1, gen;
};

// x_i = mean_i + sigma * (BD z)_i for one draw; returns whether it lies inside the box
// (BD is zero-padded to DMAX columns per row on the device, so the inner loop needs no bound)
template <int DMAX, bool KEEP>
__device__ __forceinline__ bool make_x(const SamplerArgs &a, const double *__restrict__ BD, const double (&z)[DMAX], double (&x)[DMAX]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < DMAX; ++i) {
        if (i < a.D) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < DMAX; ++j) y = fma(BD[i * DMAX + j], z[j], y);
            const double xi = fma(a.sigma, y, a.mean[i]);     // spelled out: the same bits under any -ffp-contract
            if (KEEP) x[i] = xi;
            if (a.bounded) ok = ok && xi >= a.lower[i] && xi <= a.upper[i];
        }
    }
    return ok;
}

}  // namespace alp
