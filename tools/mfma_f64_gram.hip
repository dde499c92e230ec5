// The lane map of v_mfma_f64_16x16x4_f64 as normal_body (alproj_amd/csrc/alp_point_kernels.h, K3n) relies on it, checked with
// exact small-integer data: one wave, a 64 x 24 tile R of integers in -7..7 (so that every product and sum is exact in
// float64), stored column-major with the kernel's row stride; the wave forms the Gram matrix R^T R in the three blocks 00, 01,
// 11 with the kernel's own operand reads (A = B = R[k0 + (l >> 4)][16 b + (l & 15)]) and parks it with the kernel's own C / D
// map (lane l, register e -> row (l >> 4) + 4 e, column l & 15).  The host forms R^T R in integers: any difference is a wrong
// map, not rounding.  Also run with M = 24, 17, 16, 9: the columns at or past M are read from column M - 1 and must not reach
// any element (i, j) with i <= j < M.
//   hipcc --offload-arch=gfx950 -O2 tools/mfma_f64_gram.hip -o /tmp/mfma_f64_gram && /tmp/mfma_f64_gram
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

constexpr int ROWS = 64, RS = 66, MAXM = 24;
typedef double v4d __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void gram_kernel(const double *__restrict__ tile_in, int M, double *__restrict__ out) {
    __shared__ double tile[MAXM * RS];
    const int lane = threadIdx.x;
    for (int i = lane; i < MAXM * RS; i += 64) tile[i] = tile_in[i];
    __syncthreads();
    const int kq = lane >> 4;
    const int c0 = (lane & 15) < M ? (lane & 15) : M - 1;
    const int c1 = 16 + (lane & 15) < M ? 16 + (lane & 15) : M - 1;
    const double *rd0 = tile + c0 * RS + kq, *rd1 = tile + c1 * RS + kq;
    v4d a00 = {0, 0, 0, 0}, a01 = {0, 0, 0, 0}, a11 = {0, 0, 0, 0};
    for (int k0 = 0; k0 < ROWS; k0 += 4) {
        const double f0 = rd0[k0], f1 = rd1[k0];
        a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(f0, f0, a00, 0, 0, 0);
        a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(f0, f1, a01, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(f1, f1, a11, 0, 0, 0);
    }
    for (int e = 0; e < 4; ++e) {
        const int row = kq + 4 * e, col = lane & 15;
        out[row * 32 + col] = a00[e];
        out[row * 32 + 16 + col] = a01[e];
        out[(16 + row) * 32 + 16 + col] = a11[e];
    }
}

#define CK(x)                                                                  \
    do {                                                                       \
        hipError_t e__ = (x);                                                  \
        if (e__ != hipSuccess) {                                               \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__));           \
            return 2;                                                          \
        }                                                                      \
    } while (0)

int main() {
    std::vector<double> tile(MAXM * RS, 0.0), out(32 * 32);
    unsigned s = 12345;
    std::vector<int> R(ROWS * MAXM);
    for (int k = 0; k < ROWS; ++k)
        for (int c = 0; c < MAXM; ++c) {
            s = s * 1664525u + 1013904223u;
            R[k * MAXM + c] = (int)((s >> 16) % 15) - 7;
            tile[c * RS + k] = R[k * MAXM + c];
        }
    double *d_tile = nullptr, *d_out = nullptr;
    CK(hipMalloc(&d_tile, tile.size() * sizeof(double)));
    CK(hipMalloc(&d_out, out.size() * sizeof(double)));
    CK(hipMemcpy(d_tile, tile.data(), tile.size() * sizeof(double), hipMemcpyHostToDevice));
    int bad = 0;
    for (int M : {24, 17, 16, 9}) {
        CK(hipMemset(d_out, 0, out.size() * sizeof(double)));
        hipLaunchKernelGGL(gram_kernel, dim3(1), dim3(64), 0, 0, d_tile, M, d_out);
        CK(hipGetLastError());
        CK(hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < M; ++i)
            for (int j = i; j < M; ++j) {
                long long want = 0;
                for (int k = 0; k < ROWS; ++k) want += (long long)R[k * MAXM + i] * R[k * MAXM + j];
                if (out[i * 32 + j] != (double)want) {
                    if (bad < 10) fprintf(stderr, "M = %d: G[%d][%d] = %.17g, want %lld\n", M, i, j, out[i * 32 + j], want);
                    ++bad;
                }
            }
    }
    (void)hipFree(d_tile);
    (void)hipFree(d_out);
    if (bad) {
        fprintf(stderr, "mfma_f64_gram: %d element(s) differ\n", bad);
        return 1;
    }
    printf("mfma_f64_gram ok: the Gram matrix of a 64 x 24 integer tile is exact in blocks 00, 01 and 11 at M = 24, 17, 16, 9\n");
    return 0;
}
