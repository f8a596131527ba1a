// libtvae_cluster.so: C ABI of the radial spectra (include/tvae_cluster.h, section "Radial spectra"): the windowed ring power of
// every plane of a stack, its per-group sums and the Fourier filter with a radial profile per group.  Stateless like the
// other entry points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "spectrum_kernels.hpp"

using namespace tvae_cluster;

static bool side_ok(long n) { return n >= 2 && n <= SIDE_MAX; }
static bool stack_ok(long B, long n) { return B >= 1 && B <= PLANES_MAX && side_ok(n); }
static bool flag_ok(int v) { return v == 0 || v == 1; }
// the workspace of every transform of this family: tvae_fourier_filter's
static long transform_ws_floats(int B, int n) {
    if (!stack_ok(B, n)) return 0;
    return n <= CTF_ONDIE_MAX ? 2 : 2L * B * ctf_buf_floats(n);
}

extern "C" {

int tvae_radial_rings(int n) { return side_ok(n) ? radial_rings(n) : 0; }

long tvae_ring_power_ws_floats(int B, int n) { return transform_ws_floats(B, n); }

int tvae_ring_power(const float* X, long x_stride, double* power, float* ws, long ws_floats, int B, int n, float mask_radius,
                    float mask_edge, int background, int demean, tvae_stream_t stream) {
    if (!stack_ok(B, n) || !X || !power || !ws || !flag_ok(background) || !flag_ok(demean) || !mask_ok(mask_radius, mask_edge))
        return (int)hipErrorInvalidValue;
    const long nn = (long)n * n;
    if (x_stride != 0 && x_stride < nn) return (int)hipErrorInvalidValue;
    if (!aligned8(power) || !aligned8(ws) || ws_floats < transform_ws_floats(B, n)) return (int)hipErrorInvalidValue;
    const int Rr = radial_rings(n);
    const size_t lds = ctf_lds_bytes(n);
    hipStream_t s = S(stream);
    if (n <= CTF_ONDIE_MAX) {
        const hipError_t e = allow_big_lds(ring_power_kernel<true>, lds);
        if (e != hipSuccess) return (int)e;
        ring_power_kernel<true><<<(unsigned)B, CTF_THREADS, lds, s>>>(X, x_stride, power, ws, n, Rr, mask_radius, mask_edge,
                                                                      background, demean);
    } else {
        ring_power_kernel<false><<<(unsigned)B, CTF_THREADS, lds, s>>>(X, x_stride, power, ws, n, Rr, mask_radius, mask_edge,
                                                                       background, demean);
    }
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_ring_power_groups(const double* power, const int* order, const int* seg, double* sums, int* counts, int N, int K,
                           int Rr, tvae_stream_t stream) {
    if (!power || !order || !seg || !sums || !counts || !aligned8(power) || !aligned8(sums)) return (int)hipErrorInvalidValue;
    if (N < 1 || N > PLANES_MAX || K < 1 || K > CLASSES_MAX || Rr < 1 || Rr > RINGS_MAX) return (int)hipErrorInvalidValue;
    const long tiles = (Rr + CTF_THREADS - 1) / CTF_THREADS, grid = (long)K * tiles;
    ring_group_kernel<<<(unsigned)grid, CTF_THREADS, 0, S(stream)>>>(power, order, seg, sums, counts, N, Rr, (int)tiles);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

long tvae_radial_filter_ws_floats(int B, int n) { return transform_ws_floats(B, n); }

int tvae_radial_filter(const float* X, long x_stride, const float* prof, const int* group, float* out, float* ws,
                       long ws_floats, int B, int n, int G, int interp, tvae_stream_t stream) {
    if (!stack_ok(B, n) || !X || !prof || !out || !ws || G < 1 || G > CLASSES_MAX || !flag_ok(interp))
        return (int)hipErrorInvalidValue;
    const long nn = (long)n * n;
    if (x_stride != 0 && x_stride < nn) return (int)hipErrorInvalidValue;
    if (!aligned8(ws) || ws_floats < transform_ws_floats(B, n)) return (int)hipErrorInvalidValue;
    // out is X itself, plane over plane, or does not touch it
    const float* x_end = X + (B - 1) * x_stride + nn;
    if (!(out == X && x_stride == nn) && out < x_end && X < out + (long)B * nn) return (int)hipErrorInvalidValue;
    const int Rr = radial_rings(n);
    const size_t lds = ctf_lds_bytes(n);
    hipStream_t s = S(stream);
    if (n <= CTF_ONDIE_MAX) {
        const hipError_t e = allow_big_lds(radial_filter_kernel<true>, lds);
        if (e != hipSuccess) return (int)e;
        radial_filter_kernel<true><<<(unsigned)B, CTF_THREADS, lds, s>>>(X, x_stride, prof, group, out, ws, n, Rr, G, interp);
    } else {
        radial_filter_kernel<false><<<(unsigned)B, CTF_THREADS, lds, s>>>(X, x_stride, prof, group, out, ws, n, Rr, G, interp);
    }
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
