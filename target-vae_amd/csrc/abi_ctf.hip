// libtvae_cluster.so: C ABI of the CTF kernels (include/tvae_cluster.h, last section): the transfer function from five
// coefficients per image, the per-image Fourier filter and the per-class sums of H^2.  Stateless like the other entry
// points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "ctf_kernels.hpp"

using namespace tvae_cluster;

static long spec_tiles(long n) { return (n * half_side((int)n) + CTF_THREADS - 1) / CTF_THREADS; }
static bool side_ok(long n) { return n >= 2 && n <= SIDE_MAX; }
static bool filter_shape_ok(long B, long n) { return B >= 1 && B <= PLANES_MAX && side_ok(n); }

extern "C" {

int tvae_ctf_eval(const double* coef, float* H, int N, int n, int mode, tvae_stream_t stream) {
    if (!coef || !H || !aligned8(coef) || N < 1 || N > PLANES_MAX || !side_ok(n) || (mode != 0 && mode != 1))
        return (int)hipErrorInvalidValue;
    const long tiles = spec_tiles(n), grid = (long)N * tiles;
    if (grid > GRID_MAX) return (int)hipErrorInvalidValue;
    ctf_eval_kernel<<<(unsigned)grid, CTF_THREADS, 0, S(stream)>>>(coef, H, n, (int)tiles, mode);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

long tvae_fourier_filter_ws_floats(int B, int n) {
    if (!filter_shape_ok(B, n)) return 0;
    return n <= CTF_ONDIE_MAX ? 2 : 2L * B * ctf_buf_floats(n);
}

int tvae_fourier_filter(const float* X, long x_stride, const double* coef, const float* Hp, long h_stride, float* out,
                        float* ws, long ws_floats, int B, int n, int mode, tvae_stream_t stream) {
    if (!filter_shape_ok(B, n) || !X || !out || !ws || (coef == nullptr) == (Hp == nullptr) || (mode != 0 && mode != 1))
        return (int)hipErrorInvalidValue;
    const long nn = (long)n * n, nR = (long)n * half_side(n);
    if (x_stride != 0 && x_stride < nn) return (int)hipErrorInvalidValue;
    if (Hp && h_stride != 0 && h_stride < nR) return (int)hipErrorInvalidValue;
    if (!aligned8(coef) || !aligned8(ws) || ws_floats < tvae_fourier_filter_ws_floats(B, n)) return (int)hipErrorInvalidValue;
    // out is X itself, plane over plane, or does not touch it
    const float* x_end = X + (B - 1) * x_stride + nn;
    if (!(out == X && x_stride == nn) && out < x_end && X < out + (long)B * nn) return (int)hipErrorInvalidValue;
    const size_t lds = ctf_lds_bytes(n);
    hipStream_t s = S(stream);
    if (n <= CTF_ONDIE_MAX) {
        const hipError_t e = allow_big_lds(ctf_filter_kernel<true>, lds);
        if (e != hipSuccess) return (int)e;
        ctf_filter_kernel<true><<<(unsigned)B, CTF_THREADS, lds, s>>>(X, x_stride, coef, Hp, h_stride, out, ws, n, mode);
    } else {
        ctf_filter_kernel<false><<<(unsigned)B, CTF_THREADS, lds, s>>>(X, x_stride, coef, Hp, h_stride, out, ws, n, mode);
    }
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_ctf_power(const double* coef, const int* order, const int* seg, double* D, int* counts, int N, int K, int n,
                   tvae_stream_t stream) {
    if (!coef || !order || !seg || !D || !counts || !aligned8(coef) || !aligned8(D)) return (int)hipErrorInvalidValue;
    if (N < 1 || N > PLANES_MAX || K < 1 || K > CLASSES_MAX || !side_ok(n)) return (int)hipErrorInvalidValue;
    const long tiles = spec_tiles(n), grid = (long)K * tiles;
    if (grid > GRID_MAX) return (int)hipErrorInvalidValue;
    ctf_power_kernel<<<(unsigned)grid, CTF_THREADS, 0, S(stream)>>>(coef, order, seg, D, counts, N, n, (int)tiles);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
