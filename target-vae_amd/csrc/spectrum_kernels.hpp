// Ring-indexed quantities of a stack's spectrum (include/tvae_cluster.h, section "Radial spectra"): the windowed power of every
// plane per ring, its per-group sums, and the Fourier filter with a radial profile per group.  The transforms are the stages of
// ctf_device.hpp, the code that ctf_filter_kernel runs: one 256-thread workgroup owns one plane, both buffers in LDS for
// n <= CTF_ONDIE_MAX and in the plane's own part of the workspace above.  Included by abi_spectrum.hip only.
//
// ring_power_kernel     load: x -> buffer 0 and the window w -> buffer 1 (free until stage 1), both at row stride n | 1; a thread
//                       owns the pixels tid, tid + 256, ... in every pass, so the passes need no barrier between them.
//                       demean: sum w and sum w x per thread in fp64 in ascending pixel order ((double)w (double)x is exact),
//                       the fixed tree of image_kernels.hpp over the 256 threads, mu = sum w x / sum w (0 / 0 = NaN stands);
//                       x <- (float)((double)x - mu) w.  Stages 1 and 2 leave F in buffer 0.  Then a thread = one ring: ky
//                       ascending, the kx interval of the ring in that row in exact integers (frc_first_kx, the FRC's walk),
//                       |F|^2 = re re + im im in fp64 from the fp32 coefficient, times the Hermitian weight, added in fp64.
//                       The window is evaluated per pixel and plane (window_mask: a square root and a cosine on the soft edge
//                       only).
// ring_group_kernel     a thread = one (group, ring): the valid members in ascending position, added in fp64.  The cleaned
//                       boundaries of the group are found as ctf_power_kernel finds them; the members are counted by all
//                       threads of the group's first workgroup (integers: the order does not matter).
// radial_filter_kernel  the four stages with H(ky, kx) = prof[g][ring] (nearest, the integer rule) or the fp64 linear
//                       interpolation at sqrt(ks^2 + kx^2), rounded to fp32 once, formed in registers at the multiply.  A
//                       group index outside [0, G) stores zeros and ends before the first barrier (uniform over the workgroup).
// No atomics anywhere; every output is a pure function of its own plane / group.
#pragma once
#include <hip/hip_runtime.h>

#include "ctf_device.hpp"

namespace tvae_cluster {

// 1 + the ring of the corner (h, h), h = n / 2: the rings of the whole plane
__host__ __device__ static inline int radial_rings(int n) {
    const int h = n / 2;
    return 1 + ring_of(2 * h * h);
}
constexpr int RINGS_MAX = 725;           // radial_rings(SIDE_MAX)

// fixed tree over the 256 threads' fp64 values (img_block_sum of image_kernels.hpp); the result is valid in every thread
__device__ __forceinline__ double spec_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // an earlier result has been read
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = CTF_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// frc_mask(i, j) without its square root and cosine where the answer is plain: d2 = d^2 is exact in fp64, and the rounded
// square root is monotone, so d2 < r^2 (exact: r is an fp32 value) gives d <= r and d2 > (r + e)^2 (1 + 2^-50) gives d >= r + e.
// Every other pixel -- the edge and its two borders -- takes frc_mask itself: the same bits everywhere.
__device__ __forceinline__ float window_mask(int i, int j, int n, float radius, float edge) {
    if (!(radius > 0.f)) return 1.f;
    const double c = 0.5 * (double)(n - 1);
    const double di = (double)i - c, dj = (double)j - c;
    const double d2 = di * di + dj * dj, r = (double)radius, q = r + (double)edge;
    if (d2 < r * r) return 1.f;
    if (d2 > q * q * (1.0 + 0x1p-50)) return 0.f;
    return frc_mask(i, j, n, radius, edge);
}

// grid = B.  X plane b at X + b x_stride, power[B][Rr] (fp64)
template <bool ONDIE>
__global__ __launch_bounds__(CTF_THREADS) void ring_power_kernel(const float* __restrict__ X, long x_stride,
                                                                 double* __restrict__ power, float* ws, int n, int Rr,
                                                                 float radius, float edge, int background, int demean) {
    extern __shared__ __attribute__((aligned(16))) float ctf_sm[];
    __shared__ double red[CTF_THREADS];
    float2* const tw = reinterpret_cast<float2*>(ctf_sm);
    const int R = half_side(n), ld = ctf_ld(n), ldx = n | 1;
    const long buf = ctf_buf_floats(n);
    const size_t b = blockIdx.x;
    float* const buf0 = ONDIE ? ctf_sm + 2 * n : ws + b * 2 * buf;
    float* const buf1 = buf0 + buf;
    const CtfLane L = ctf_lane();
    const bool masked = radius > 0.f;

    dft_twiddles(tw, n, CTF_THREADS);
    {
        const float* x = X + b * x_stride;
        double sw = 0.0, swx = 0.0;
        for (int e = L.tid; e < n * n; e += CTF_THREADS) {
            const int i = e / n, j = e - i * n;
            const float m = window_mask(i, j, n, radius, edge);
            const float w = (masked && background) ? 1.f - m : m;
            const float v = x[e];
            if (demean) {
                sw += (double)w;
                swx += (double)w * (double)v;
            }
            buf0[i * ldx + j] = v;
            buf1[i * ldx + j] = w;
        }
        if (demean) {
            sw = spec_block_sum(sw, red);
            swx = spec_block_sum(swx, red);
            const double mu = swx / sw;
            for (int e = L.tid; e < n * n; e += CTF_THREADS) {
                const int i = e / n, j = e - i * n;
                buf0[i * ldx + j] = (float)((double)buf0[i * ldx + j] - mu) * buf1[i * ldx + j];
            }
        } else {
            for (int e = L.tid; e < n * n; e += CTF_THREADS) {
                const int i = e / n, j = e - i * n;
                buf0[i * ldx + j] *= buf1[i * ldx + j];
            }
        }
    }
    __syncthreads();
    ctf_rows(tw, buf0, buf1, n, R, ld, L.wave, L.l31, L.khalf);
    __syncthreads();
    ctf_columns<-1>(tw, buf1, buf0, n, R, ld, L.wave, L.l31, L.khalf);
    __syncthreads();

    // a thread = one ring.  Ring r = 4 (tid & 63) + (tid >> 6) (+ 256 ...): a wave holds every fourth ring, so the ring that is
    // tangent to a row -- the longest interval of that row, which its whole wave waits for -- is another wave's from row to row
    const float* fr = buf0;
    const float* fi = buf0 + (size_t)n * ld;
    for (int r = 4 * (L.tid & 63) + (L.tid >> 6); r < Rr; r += CTF_THREADS) {
        const int lo2 = (2 * r - 1) * (2 * r - 1), hi2 = (2 * r + 1) * (2 * r + 1);
        double sum = 0.0;
        for (int row = 0; row < n; ++row) {                   // numpy's fftfreq order: 0, 1, ..., then the negative ones
            const int ky = row < (n + 1) / 2 ? row : row - n;
            const int k4 = 4 * ky * ky;
            const int a = r == 0 ? 0 : frc_first_kx(lo2 - k4);
            const int e = min(frc_first_kx(hi2 - k4), R);
            for (int kx = a; kx < e; ++kx) {
                const double wk = (kx == 0 || 2 * kx == n) ? 1.0 : 2.0;
                const size_t at = (size_t)row * ld + kx;
                const double re = (double)fr[at], im = (double)fi[at];
                sum += wk * (re * re + im * im);
            }
        }
        power[b * Rr + r] = sum;
    }
}

// grid = K * tiles (tile fastest), tiles = ceil(Rr / 256).  power[N][Rr] -> sums[K][Rr] (fp64), counts[K] (written by tile 0)
__global__ __launch_bounds__(CTF_THREADS) void ring_group_kernel(const double* __restrict__ power, const int* __restrict__ order,
                                                                 const int* __restrict__ seg, double* __restrict__ sums,
                                                                 int* __restrict__ counts, int N, int Rr, int tiles) {
    __shared__ int red[CTF_THREADS];
    const int k = blockIdx.x / tiles, tile = blockIdx.x - k * tiles;
    // cleaned boundaries of group k: min(max(0, seg[0], ..., seg[k]), N) and the same with seg[k + 1]
    int m = 0;
    for (int q = threadIdx.x; q <= k; q += CTF_THREADS) m = max(m, seg[q]);
    red[threadIdx.x] = m;
    __syncthreads();
#pragma unroll
    for (int s = CTF_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const int run = red[0];
    const int sk = min(run, N), ek = min(max(run, seg[k + 1]), N);
    if (tile == 0) {                                          // (the same for the whole workgroup)
        int c = 0;
        for (int p = sk + (int)threadIdx.x; p < ek; p += CTF_THREADS) {
            const int id = order[p];
            c += id >= 0 && id < N;
        }
        __syncthreads();                                      // red[0] has been read
        red[threadIdx.x] = c;
        __syncthreads();
#pragma unroll
        for (int s = CTF_THREADS / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) counts[k] = red[0];
    }
    const int r = tile * CTF_THREADS + threadIdx.x;
    if (r >= Rr) return;
    double sum = 0.0;
    for (int p = sk; p < ek; ++p) {
        const int id = order[p];
        if (id < 0 || id >= N) continue;
        sum += power[(size_t)id * Rr + r];
    }
    sums[(size_t)k * Rr + r] = sum;
}

// H(ky, kx) of the profile p[Rr]
__device__ __forceinline__ float radial_value(const float* __restrict__ p, int ky, int kx, int n, int Rr, int interp) {
    const int ks = ky < (n + 1) / 2 ? ky : ky - n;
    const int s2 = ks * ks + kx * kx;
    if (interp == 0) return p[ring_of(s2)];
    const double s = sqrt((double)s2);
    const int r0 = min((int)floor(s), Rr - 2);
    const double p0 = (double)p[r0], p1 = (double)p[r0 + 1];
    return (float)fma(p1 - p0, s - (double)r0, p0);
}

// grid = B.  X plane b at X + b x_stride, prof[G][Rr], group[B] or null (group 0 for all), out[B][n][n] (may be X)
template <bool ONDIE>
__global__ __launch_bounds__(CTF_THREADS) void radial_filter_kernel(const float* X, long x_stride,
                                                                    const float* __restrict__ prof,
                                                                    const int* __restrict__ group, float* out, float* ws,
                                                                    int n, int Rr, int G, int interp) {
    extern __shared__ __attribute__((aligned(16))) float ctf_sm[];
    float2* const tw = reinterpret_cast<float2*>(ctf_sm);
    const int R = half_side(n), ld = ctf_ld(n);
    const long buf = ctf_buf_floats(n);
    const size_t b = blockIdx.x;
    float* const buf0 = ONDIE ? ctf_sm + 2 * n : ws + b * 2 * buf;
    float* const buf1 = buf0 + buf;
    const CtfLane L = ctf_lane();
    float* const o = out + b * (size_t)n * n;
    const int g = group ? group[b] : 0;
    if (g < 0 || g >= G) {                                    // the same for every thread of the workgroup
        for (int e = L.tid; e < n * n; e += CTF_THREADS) o[e] = 0.f;
        return;
    }
    const float* p = prof + (size_t)g * Rr;

    dft_twiddles(tw, n, CTF_THREADS);
    ctf_load_plane(X + b * x_stride, buf0, n, L.tid);
    __syncthreads();
    ctf_rows(tw, buf0, buf1, n, R, ld, L.wave, L.l31, L.khalf);
    __syncthreads();
    ctf_columns<-1>(tw, buf1, buf0, n, R, ld, L.wave, L.l31, L.khalf);
    __syncthreads();
    ctf_multiply(buf0, n, R, ld, L.tid, [=](int ky, int kx, int) { return radial_value(p, ky, kx, n, Rr, interp); });
    __syncthreads();
    ctf_columns<1>(tw, buf0, buf1, n, R, ld, L.wave, L.l31, L.khalf);
    __syncthreads();
    ctf_rows_back(tw, buf1, o, n, R, ld, L.wave, L.l31, L.khalf);
}

}  // namespace tvae_cluster
