// Per-image Fourier filtering with a real transfer function (include/tvae_cluster.h, last section): the CTF evaluated from five
// fp64 coefficients per image, the filter out = Re IDFT(H DFT(x)) of every plane of a stack, and the per-class sums of H^2.
//
// ctf_value             H(ky, kx) of one coefficient row.  q = (ks^2 + kx^2) / n^2 from the exact integer numerator (one fp64
//                       division), t = c2 q + c3 q^2 in fp64 and reduced to t - rint(t) there, sin and cos of 2 pi t by
//                       sincospi in fp64 on the exact argument 2 t, c0 sin + c1 cos in fp64 and rounded to fp32 ONCE, the
//                       envelope expf of the fp32 rounding of -c4 q (1 ulp, plus |c4 q| 2^-24 exp(-c4 q) <= 0.37 2^-24 from the
//                       argument for c4 q >= 0), one fp32 product: about 3 2^-24 (|c0| + |c1|), inside the contract's 8.
//                       Every kernel here calls this one function: an image's H is the same bits wherever it is formed.
// ctf_eval_kernel       a thread = one (ky, kx) of one row.
// ctf_filter_kernel     ONE 256-thread workgroup (four waves) owns ONE plane from load to store; a direct DFT in four stages
//                       on v_mfma_f32_32x32x2_f32 (the fragment layout: cluster_common.hpp):
//                         1 rows          G(i, kx)  = sum_j  x(i, j) e^{-2 pi i kx j / n}              2 MFMAs per k step
//                         2 columns       F(ky, kx) = sum_i  e^{-2 pi i ky i / n} G(i, kx)             4
//                           multiply      F *= H(ky, kx) w_kx, H formed in registers (or read from the caller's plane)
//                         3 columns back  P(i, kx)  = sum_ky e^{+2 pi i ky i / n} F(ky, kx)            4
//                         4 rows back     out(i, j) = n^-2 sum_kx Re(P(i, kx) e^{+2 pi i kx j / n})    2
//                       A wave walks 32 x 32 output tiles (tile = wave, wave + 4, ...), the whole reduction of a tile in its
//                       registers.  The twiddle operand of every stage is NOT staged: a lane reads it from the table of the n
//                       values (cos, sin)(2 pi t / n) at t = (a k) mod n, kept in integers (tw_advance by 2 a mod n per step), so
//                       no argument is ever reduced in floating point.  The data operand comes from one of two buffers of
//                       2 n ld floats (re plane, im plane; row stride ld = (n / 2 + 1) | 1, odd: the A-fragment reads of 32
//                       consecutive rows at a fixed k and the B-fragment reads of 32 consecutive columns are conflict-free):
//                       buffer 0 holds x (row stride n | 1), then F; buffer 1 holds G, then P.  Rows, columns and k outside
//                       the plane are PREDICATED zeros, never loaded, and nothing outside the plane is stored.
//                       Routes: ONDIE (n <= CTF_ONDIE_MAX = 128) keeps both buffers in LDS, 8 n + 16 n ld bytes (134 144 at
//                       n = 128: one workgroup per CU): in coefficient mode neither the spectrum nor H is ever in HBM.  Any
//                       larger n runs the SAME code on the plane's own 4 n ld floats of the caller's workspace (LDS holds the
//                       table only); a workgroup reads only what it wrote itself, behind workgroup barriers.
//                       The plane is read completely before the first barrier and written after the last: out may be X.
//                       The stages themselves are the __device__ functions of ctf_device.hpp, which the ring-power and
//                       radial-filter kernels (spectrum_kernels.hpp) call as well: one body of code, the same bits.
// ctf_power_kernel     a thread = one (ky, kx) of class k: the members in ascending position, H_i^2 formed and added in fp64.
//                       The cleaned boundaries min(max(0, seg[0 .. k]), N) of its class are found by the workgroup itself (a
//                       strided maximum and a fixed tree; a maximum does not depend on the order), the rule of avg_seg_kernel.
// No atomics anywhere; every output is a pure function of its own plane / class.
#pragma once
#include <hip/hip_runtime.h>

#include "ctf_device.hpp"

namespace tvae_cluster {

// (ctf_value itself is defined in ctf_device.hpp: tvae_template_ctf_power, another unit, forms the same H)
// grid = N * tiles (tile fastest), tiles = ceil(n R / 256).  H[N][n][R]
__global__ __launch_bounds__(CTF_THREADS) void ctf_eval_kernel(const double* __restrict__ coef, float* __restrict__ H, int n,
                                                               int tiles, int mode) {
    const int R = half_side(n);
    const unsigned row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const int e = (int)tile * CTF_THREADS + threadIdx.x;
    if (e >= n * R) return;
    const int ky = e / R, kx = e - ky * R;
    H[(size_t)row * n * R + e] = ctf_value(coef + 5 * (size_t)row, ky, kx, n, mode);
}

// grid = B.  X plane b at X + b x_stride, out[B][n][n] (may be X); exactly one of coef [B][5] and Hp (plane b at Hp + b h_stride)
template <bool ONDIE>
__global__ __launch_bounds__(CTF_THREADS) void ctf_filter_kernel(const float* X, long x_stride,
                                                                 const double* __restrict__ coef,
                                                                 const float* __restrict__ Hp, long h_stride, float* out,
                                                                 float* ws, int n, int mode) {
    extern __shared__ __attribute__((aligned(16))) float ctf_sm[];
    float2* const tw = reinterpret_cast<float2*>(ctf_sm);
    const int R = half_side(n), ld = ctf_ld(n);
    const long buf = ctf_buf_floats(n);
    const size_t b = blockIdx.x;
    float* const buf0 = ONDIE ? ctf_sm + 2 * n : ws + b * 2 * buf;
    float* const buf1 = buf0 + buf;
    const CtfLane L = ctf_lane();

    dft_twiddles(tw, n, CTF_THREADS);
    ctf_load_plane(X + b * x_stride, buf0, n, L.tid);
    __syncthreads();
    ctf_rows(tw, buf0, buf1, n, R, ld, L.wave, L.l31, L.khalf);                  // stage 1: x (buffer 0) -> G (buffer 1)
    __syncthreads();
    ctf_columns<-1>(tw, buf1, buf0, n, R, ld, L.wave, L.l31, L.khalf);           // stage 2: G -> F (buffer 0, x is no longer needed)
    __syncthreads();
    {
        const double* cf = coef ? coef + 5 * b : nullptr;
        const float* hp = Hp ? Hp + b * h_stride : nullptr;
        ctf_multiply(buf0, n, R, ld, L.tid, [=](int ky, int kx, int e) {
            if (cf) return ctf_value(cf, ky, kx, n, mode);
            const float h = hp[e];
            return mode == 1 ? (h < 0.f ? -1.f : 1.f) : h;
        });
    }
    __syncthreads();
    ctf_columns<1>(tw, buf0, buf1, n, R, ld, L.wave, L.l31, L.khalf);            // stage 3: F -> P (buffer 1)
    __syncthreads();
    ctf_rows_back(tw, buf1, out + b * (size_t)n * n, n, R, ld, L.wave, L.l31, L.khalf);     // stage 4
}

// grid = K * tiles (tile fastest), tiles = ceil(n R / 256).  D[K][n][R] (fp64), counts[K] (written by tile 0)
__global__ __launch_bounds__(CTF_THREADS) void ctf_power_kernel(const double* __restrict__ coef,
                                                                const int* __restrict__ order, const int* __restrict__ seg,
                                                                double* __restrict__ D, int* __restrict__ counts, int N,
                                                                int n, int tiles) {
    __shared__ int red[CTF_THREADS];
    const int R = half_side(n);
    const int k = blockIdx.x / tiles, tile = blockIdx.x - k * tiles;
    // cleaned boundaries of class k: min(max(0, seg[0], ..., seg[k]), N) and the same with seg[k + 1]
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
    if (tile == 0 && threadIdx.x == 0) {
        int c = 0;
        for (int p = sk; p < ek; ++p) {
            const int id = order[p];
            c += id >= 0 && id < N;
        }
        counts[k] = c;
    }
    const int e = tile * CTF_THREADS + threadIdx.x;
    if (e >= n * R) return;
    const int ky = e / R, kx = e - ky * R;
    double sum = 0.0;
    for (int p = sk; p < ek; ++p) {
        const int id = order[p];
        if (id < 0 || id >= N) continue;
        const double h = (double)ctf_value(coef + 5 * (size_t)id, ky, kx, n, 0);
        sum += h * h;
    }
    D[(size_t)k * n * R + e] = sum;
}

}  // namespace tvae_cluster
