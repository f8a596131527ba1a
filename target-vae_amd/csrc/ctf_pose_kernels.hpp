// The CTF in the template of the pose searches (include/tvae_cluster.h, section "CTF in the template"): what joins the CTF
// filter, the pose tables and the weighted average under the model Y_i = H_i (*) P_j + noise.  Included by abi_ctf_pose.hip only.
//
// template_ctf_power_kernel  ONE 256-thread workgroup owns ONE (image, slot, angle) from template to sum.  Per channel:
//                            the template of tvae_pose_refine on the frame r, q = 0 .. n - 1, mask included, by
//                            refine_angle_pose / refine_position / refine_build_template<0> (refine_device.hpp) straight into
//                            buffer 0 at row stride n | 1 -- the layout ctf_load_plane gives a plane, and bit for bit the centre
//                            window of that kernel's extended template; stages 1 and 2 of the filter's DFT (ctf_device.hpp, the
//                            code tvae_ring_power runs) leave F in buffer 0; then thread t adds the coefficients
//                            e = ky R + kx = t, t + 256, ... (ascending ky index, then kx) to ONE fp64 chain that runs on through
//                            the channels in ascending order:
//                                H = ctf_value(coef[i]) (fp32, in registers),  hh = (double)H (double)H             (exact),
//                                p = (double)re (double)re + (double)im (double)im                  (one rounding, the sum),
//                                chain = chain + w_kx (hh p)                           (w_kx = 1 or 2: exact; two roundings).
//                            The 256 chains go through the fixed tree of tvae_ring_power's demean (s[t] += s[t + w], w = 128,
//                            64, ..., 1), the total is divided by (double)(n n) and rounded to fp32 once.
//                            Neither H, T nor the spectrum reaches memory: both buffers are LDS (8 n + 16 n ld bytes, 134 144
//                            at n = 128, one workgroup per CU there: the budget of ring_power_kernel) and the workspace is the
//                            filter's untouched 2-float dummy.  A slot outside [0, K) stores 0 and ends before the first
//                            barrier (uniform over the workgroup) with nothing of ref read.  A template that is out of frame
//                            throughout is exact zeros, its spectrum is, and the sum is exact 0 for finite H.
// ctf_power_weighted_kernel  ctf_power_kernel over E entries with weights: a thread = one (ky, kx) of class k, the live
//                            entries in ascending e, (double)w_e ((double)H (double)H) formed (one rounding: H^2 is exact) and
//                            added in fp64.  The cleaned boundaries with E as the bound are found by the workgroup itself, as
//                            ctf_power_kernel finds them; thread 0 of the class's tile 0 adds the live weights in ascending e
//                            in fp64 and counts them.
// No atomics anywhere; every output is a pure function of its own (image, slot, angle) / class.
#pragma once
#include <hip/hip_runtime.h>

// (the order matters: the stages and ctf_value are compiled as abi_ctf.hip and abi_spectrum.hip compile them; refine_device.hpp
// then turns fp contraction off for itself and for what follows)
#include "ctf_device.hpp"
#include "refine_device.hpp"

#pragma clang fp contract(off)

namespace tvae_cluster {

constexpr int TCP_M_MAX = TVAE_CLASSIFY_MAX_CANDIDATES;
constexpr long CPW_E_MAX = 1L << 30;

// fixed tree over the 256 threads' fp64 values (spec_block_sum of spectrum_kernels.hpp); the result is valid in thread 0
__device__ __forceinline__ double tcp_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = CTF_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// grid = N * M * NA (angle fastest, then slot).  cand [N][M], ref [K][C][n][n], coef [N][5]; ppc [N][M][NA]
__global__ __launch_bounds__(CTF_THREADS) void template_ctf_power_kernel(
    const float* __restrict__ theta, const float* __restrict__ dx, const int* __restrict__ cand,
    const float* __restrict__ ref, const double* __restrict__ coef, float* __restrict__ ppc, int C, int n, int K, int M,
    int A, float t_scale, float dtheta, float mask_radius, float mask_edge) {
    static_assert(CTF_THREADS == REFINE_TILE, "the template is built by the workgroup of the DFT stages");
    extern __shared__ __attribute__((aligned(16))) float ctf_sm[];
    __shared__ double red[CTF_THREADS];
    float2* const tw = reinterpret_cast<float2*>(ctf_sm);
    const int R = half_side(n), ld = ctf_ld(n);
    float* const buf0 = ctf_sm + 2 * n;
    float* const buf1 = buf0 + ctf_buf_floats(n);
    const CtfLane L = ctf_lane();
    const int NA = 2 * A + 1;
    const size_t b = blockIdx.x;
    const int img = (int)(b / ((size_t)M * NA));
    const int rest = (int)(b - (size_t)img * M * NA);
    const int m = rest / NA, ai = rest - m * NA;
    const int k = cand[(size_t)img * M + m];
    if (k < 0 || k >= K) {                                    // the same for every thread of the workgroup
        if (L.tid == 0) ppc[b] = 0.f;
        return;
    }
    const RefinePose pose = refine_angle_pose(theta, dx, img, ai, A, t_scale, dtheta);
    const double* __restrict__ cf = coef + 5 * (size_t)img;
    const size_t nn = (size_t)n * n;
    const float* fr = buf0;
    const float* fi = buf0 + (size_t)n * ld;

    dft_twiddles(tw, n, CTF_THREADS);
    double chain = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        __syncthreads();                                      // the spectrum of the channel before has been read
        refine_build_template<0>(buf0, ref + ((size_t)k * C + ch) * nn, n, pose, mask_radius, mask_edge, L.tid);
        __syncthreads();
        ctf_rows(tw, buf0, buf1, n, R, ld, L.wave, L.l31, L.khalf);               // stage 1: T (buffer 0) -> G (buffer 1)
        __syncthreads();
        ctf_columns<-1>(tw, buf1, buf0, n, R, ld, L.wave, L.l31, L.khalf);        // stage 2: G -> F (buffer 0)
        __syncthreads();
        for (int e = L.tid; e < n * R; e += CTF_THREADS) {
            const int ky = e / R, kx = e - ky * R;
            const double h = (double)ctf_value(cf, ky, kx, n, 0);
            const double wk = (kx == 0 || 2 * kx == n) ? 1.0 : 2.0;
            const size_t at = (size_t)ky * ld + kx;
            const double re = (double)fr[at], im = (double)fi[at];
            const double p = re * re + im * im;               // (the squares are exact)
            chain = chain + wk * ((h * h) * p);
        }
    }
    const double total = tcp_block_sum(chain, red);
    if (L.tid == 0) ppc[b] = (float)(total / (double)(n * n));
}

// grid = K * tiles (tile fastest), tiles = ceil(n R / 256).  coef [N][5], img, w [E], seg [K + 1]; D[K][n][R] (fp64), and
// wsum[K] (fp64) and counts[K] written by tile 0
__global__ __launch_bounds__(CTF_THREADS) void ctf_power_weighted_kernel(const double* __restrict__ coef,
                                                                         const int* __restrict__ img,
                                                                         const float* __restrict__ w,
                                                                         const int* __restrict__ seg, double* __restrict__ D,
                                                                         double* __restrict__ wsum, int* __restrict__ counts,
                                                                         int N, int E, int n, int tiles) {
    __shared__ int red[CTF_THREADS];
    const int R = half_side(n);
    const int k = blockIdx.x / tiles, tile = blockIdx.x - k * tiles;
    // cleaned boundaries of class k: min(max(0, seg[0], ..., seg[k]), E) and the same with seg[k + 1]
    int mx = 0;
    for (int q = threadIdx.x; q <= k; q += CTF_THREADS) mx = max(mx, seg[q]);
    red[threadIdx.x] = mx;
    __syncthreads();
#pragma unroll
    for (int s = CTF_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const int run = red[0];
    const int sk = min(run, E), ek = min(max(run, seg[k + 1]), E);
    if (tile == 0 && threadIdx.x == 0) {
        int c = 0;
        double W = 0.0;
        for (int e = sk; e < ek; ++e) {
            const int id = img[e];
            const float wv = w[e];
            if (id < 0 || id >= N || !(wv - wv == 0.f) || !(wv > 0.f)) continue;          // dead: nothing of it counts
            c += 1;
            W = W + (double)wv;
        }
        counts[k] = c;
        wsum[k] = W;
    }
    const int el = tile * CTF_THREADS + threadIdx.x;
    if (el >= n * R) return;
    const int ky = el / R, kx = el - ky * R;
    double sum = 0.0;
    for (int e = sk; e < ek; ++e) {
        const int id = img[e];
        const float wv = w[e];
        if (id < 0 || id >= N || !(wv - wv == 0.f) || !(wv > 0.f)) continue;
        const double h = (double)ctf_value(coef + 5 * (size_t)id, ky, kx, n, 0);
        sum = sum + (double)wv * (h * h);
    }
    D[(size_t)k * n * R + el] = sum;
}

}  // namespace tvae_cluster
