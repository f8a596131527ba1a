// Pose refinement against the class averages (libtvae_cluster.so): the inverse of the map of align_kernels.hpp.  The class
// average of an image's class is rendered into the image's frame at NA angles around the predicted one, on a grid extended by
// S pixels to every side, and compared with the image at the NS x NS whole-pixel shifts: num = sum P Y and pp = sum P^2 per
// candidate (angle, sy, sx), yy = sum Y^2 per image; the cosine num / sqrt(pp yy) picks the pose.  include/tvae_cluster.h
// states the definition.  Included by abi_refine.hip only.
//
// refine_corr_kernel<S>  a workgroup = one (image, angle), 256 threads.  Per channel the image plane and the extended template
//                        (NA (n + 2S)^2 C bilinear samples per image instead of NA NS^2 n^2 C) sit in LDS, row strides odd:
//                        lanes run along rows, and an odd stride puts 32 rows on 32 banks.
//                        num: thread (sy, g) owns the rows r = g, g + G, ... of the frame for the row shift sy and keeps the NS
//                        sums over sx in registers.  Along a row the NS template values under the window slide through a
//                        register ring (one LDS read of T and one of Y per NS multiply-adds; S is a template argument so that
//                        the ring and the sums are registers).  The G partial sums of a candidate are added in ascending g.
//                        pp: the sum of T^2 over a window is separable: R2[re][sx] = the sum over the n columns of the window
//                        of row re of the extended template, then pp[sy][sx] = the sum of R2 over the n rows of the window:
//                        (n + 2S) NS n + NS^2 n operations instead of NS^2 n^2.
//                        The workgroup of the first angle also forms yy.
// refine_select_kernel   a thread = an image: the scores of its NA NS^2 candidates in ascending (a, sy, sx) from the tables,
//                        in fp64 from the three fp32 sums, the selection rule of the header, and the new pose.
// No atomics; a candidate's sums are fixed chains whose order depends on (n, S, C) only.
#pragma once
#include <hip/hip_runtime.h>

#include "cluster_common.hpp"

// The definition rounds every product and sum on its own (theta + a dtheta above all: the refined angle is compared bit for
// bit).  The runtime's __fmul_rn and __fadd_rn are plain operators that the compiler may still fuse after inlining, so the
// operations of this file are its own, defined under contract(off): every fused multiply-add below is an fmaf.
#pragma clang fp contract(off)

namespace tvae_cluster {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }       // (correctly rounded: the build's default)

constexpr int REFINE_TILE = 256;        // threads per workgroup
constexpr int REFINE_SIDE_MAX = 128;     // n: one image plane and one extended template fit the 160 KB of LDS
constexpr int REFINE_C_MAX = 16;
constexpr int REFINE_A_MAX = 32;
constexpr int REFINE_S_MAX = 8;

// row stride of a plane of `side` columns in LDS: odd
__host__ __device__ static inline int refine_stride(int side) { return side | 1; }

// G: the row groups of a row shift.  At most REFINE_TILE / NS (one thread per (sy, g)); as few rows per group as that
// allows, and then no more groups than those rows need.  1 <= G <= n.
__host__ __device__ static inline int refine_groups(int n, int NS) {
    const int cap = REFINE_TILE / NS;
    const int rows = (n + cap - 1) / cap;
    return (n + rows - 1) / rows;
}

// floats of LDS: the image plane and the template (the partial sums [NS][G][NS] take their place at the end), R2 and the 256
// partials of yy
static inline size_t refine_lds_floats(int n, int S) {
    const int NS = 2 * S + 1, ne = n + 2 * S;
    const size_t planes = (size_t)n * refine_stride(n) + (size_t)ne * refine_stride(ne);
    const size_t parts = (size_t)NS * refine_groups(n, NS) * NS;
    return (planes > parts ? planes : parts) + (size_t)ne * NS + REFINE_TILE;
}

// grid = N * NA (angle fastest).  num, pp [N][NA][NS][NS], yy [N]
template <int S>
__global__ __launch_bounds__(REFINE_TILE) void refine_corr_kernel(
    const float* __restrict__ Y, const float* __restrict__ theta, const float* __restrict__ dx,
    const int* __restrict__ cls, const float* __restrict__ ref, float* __restrict__ num, float* __restrict__ pp,
    float* __restrict__ yy, int C, int n, int K, int A, float t_scale, float dtheta, float mask_radius,
    float mask_edge) {
    constexpr int NS = 2 * S + 1;
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int NA = 2 * A + 1;
    const int img = blockIdx.x / NA, ai = blockIdx.x - img * NA;
    float* __restrict__ numo = num + ((size_t)img * NA + ai) * (NS * NS);
    float* __restrict__ ppo = pp + ((size_t)img * NA + ai) * (NS * NS);
    const int k = cls[img];
    if (k < 0 || k >= K) {                                    // uniform over the workgroup, before any barrier
        for (int e = tid; e < NS * NS; e += REFINE_TILE) {
            numo[e] = 0.f;
            ppo[e] = 0.f;
        }
        if (ai == 0 && tid == 0) yy[img] = 0.f;
        return;
    }
    const int ne = n + 2 * S, ystride = refine_stride(n), tstride = refine_stride(ne);
    const int G = refine_groups(n, NS);
    float* __restrict__ ys = lds;                             // [n][ystride]
    float* __restrict__ ts = ys + n * ystride;                // [ne][tstride]
    float* __restrict__ pn = lds;                             // [NS][G][NS], once ys and ts are done with
    const size_t planes = (size_t)n * ystride + (size_t)ne * tstride, parts = (size_t)NS * G * NS;
    float* __restrict__ r2s = lds + (planes > parts ? planes : parts);   // [ne][NS]
    float* __restrict__ red = r2s + ne * NS;                  // [REFINE_TILE]

    // the pose of this angle: every operation rounded to fp32 on its own
    const float th = add_rn(theta[img], mul_rn((float)(ai - A), dtheta));
    const float c = cosf(th), s = sinf(th);
    const float tx = mul_rn(t_scale, dx[2 * (size_t)img]), ty = mul_rn(t_scale, dx[2 * (size_t)img + 1]);
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const bool masked = mask_radius > 0.f;
    const size_t nn = (size_t)n * n;

    const bool worker = tid < NS * G;
    const int syi = tid / G, g = tid - syi * G;               // the row shift sy = syi - S and the row group of this thread
    float acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.f;

    for (int ch = 0; ch < C; ++ch) {
        const float* __restrict__ Yp = Y + ((size_t)img * C + ch) * nn;
        const float* __restrict__ Rp = ref + ((size_t)k * C + ch) * nn;
        if (ch > 0) __syncthreads();                          // the previous channel's planes are still being read
        for (int e = tid; e < n * n; e += REFINE_TILE) {
            const int r = e / n, q = e - r * n;
            ys[r * ystride + q] = Yp[e];
        }
        for (int e = tid; e < ne * ne; e += REFINE_TILE) {
            const int re = e / ne, qe = e - re * ne;
            const float x0 = fmaf((float)(qe - S), step, -1.f);
            const float x1 = fmaf(-(float)(re - S), step, 1.f);
            const float v0 = x0 - tx, v1 = x1 - ty;
            const float u0 = fmaf(v0, c, -mul_rn(v1, s));
            const float u1 = fmaf(v0, s, mul_rn(v1, c));
            const float col = mul_rn(u0 + 1.f, half);
            const float row = mul_rn(1.f - u1, half);
            float v = bilinear_zero_border(Rp, n, col, row, true);
            if (masked) {
                // out of frame (NaN and +-inf among it) stays an exact 0 whatever the mask would be there
                const bool in = inside_frame(col, row, n);
                const double d = sqrt((double)u0 * (double)u0 + (double)u1 * (double)u1) * (0.5 * (double)(n - 1));
                v = in ? mul_rn(soft_mask(d, mask_radius, mask_edge), v) : 0.f;
            }
            ts[re * tstride + qe] = v;
        }
        __syncthreads();
        if (worker) {
            for (int r = g; r < n; r += G) {
                const float* __restrict__ trow = ts + (r + 2 * S - syi) * tstride;   // T_a[r - sy], extended row index
                const float* __restrict__ yrow = ys + r * ystride;
                float ring[NS];                               // T[q + j] at slot (q + j) % NS
#pragma unroll
                for (int j = 0; j < NS; ++j) ring[j] = trow[j];
                for (int q0 = 0; q0 < n; q0 += NS) {
#pragma unroll
                    for (int u = 0; u < NS; ++u) {
                        const int q = q0 + u;
                        if (q < n) {                          // (uniform)
                            const float y = yrow[q];
#pragma unroll
                            for (int sxi = 0; sxi < NS; ++sxi)    // P(r, q) = T[r - sy][q - sx]: column q + 2S - sxi
                                acc[sxi] = fmaf(ring[(u + 2 * S - sxi) % NS], y, acc[sxi]);
                            if (q + NS < ne) ring[u] = trow[q + NS];
                        }
                    }
                }
            }
        }
        for (int e = tid; e < ne * NS; e += REFINE_TILE) {    // the same thread owns R2[e] in every channel
            const int re = e / NS, sxi = e - re * NS;
            const float* __restrict__ trow = ts + re * tstride + (2 * S - sxi);
            float a = ch == 0 ? 0.f : r2s[e];
            for (int q = 0; q < n; ++q) {
                const float v = trow[q];
                a = fmaf(v, v, a);
            }
            r2s[e] = a;
        }
    }
    __syncthreads();
    if (worker) {
#pragma unroll
        for (int sxi = 0; sxi < NS; ++sxi) pn[(syi * G + g) * NS + sxi] = acc[sxi];
    }
    __syncthreads();
    for (int e = tid; e < NS * NS; e += REFINE_TILE) {
        const int sy_i = e / NS, sxi = e - sy_i * NS;
        float a = pn[(sy_i * G) * NS + sxi];
        for (int gg = 1; gg < G; ++gg) a += pn[(sy_i * G + gg) * NS + sxi];
        numo[e] = a;
        float p = 0.f;
        for (int r = 0; r < n; ++r) p += r2s[(r + 2 * S - sy_i) * NS + sxi];
        ppo[e] = p;
    }
    if (ai == 0) {                                            // (uniform)
        float a = 0.f;
        for (int ch = 0; ch < C; ++ch) {
            const float* __restrict__ Yp = Y + ((size_t)img * C + ch) * nn;
            for (int e = tid; e < n * n; e += REFINE_TILE) {
                const float v = Yp[e];
                a = fmaf(v, v, a);
            }
        }
        red[tid] = a;
        __syncthreads();
        for (int w = REFINE_TILE / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) yy[img] = red[0];
    }
}

__device__ __forceinline__ bool refine_finite(float x) { return x - x == 0.f; }

// score of one candidate from its three sums: fp64, rounded to fp32 once; exactly 0 where pp or yy is 0
__device__ __forceinline__ float refine_score(float nu, float p, float y) {
    if (p == 0.f || y == 0.f) return 0.f;
    return (float)__ddiv_rn((double)nu, __dsqrt_rn(__dmul_rn((double)p, (double)y)));   // each correctly rounded
}

// grid = ceil(N / 256).  theta_out [N], dx_out [N][2], score [N][2], best [N][3]
__global__ __launch_bounds__(REFINE_TILE) void refine_select_kernel(
    const float* __restrict__ theta, const float* __restrict__ dx, const int* __restrict__ cls,
    const float* __restrict__ num, const float* __restrict__ pp, const float* __restrict__ yy,
    float* __restrict__ theta_out, float* __restrict__ dx_out, float* __restrict__ score, int* __restrict__ best, int N,
    int n, int K, int A, int S, float t_scale, float dtheta) {
    const int i = blockIdx.x * REFINE_TILE + threadIdx.x;
    if (i >= N) return;
    const int NS = 2 * S + 1, NA = 2 * A + 1, cand = NA * NS * NS;
    const float th = theta[i], d0 = dx[2 * (size_t)i], d1 = dx[2 * (size_t)i + 1];
    const int k = cls[i];
    float sc = 0.f, sb = 0.f;
    int bi = (A * NS + S) * NS + S;                           // the centre
    if (k >= 0 && k < K) {
        const float* __restrict__ nu = num + (size_t)i * cand;
        const float* __restrict__ p = pp + (size_t)i * cand;
        const float y = yy[i];
        const float centre = refine_score(nu[bi], p[bi], y);
        const float ninf = -__builtin_inff();
        bool any = refine_finite(centre);
        float bv = any ? centre : ninf;
        for (int e = 0; e < cand; ++e) {
            const float v = refine_score(nu[e], p[e], y);
            if (refine_finite(v) && v > bv) {
                bv = v;
                bi = e;
                any = true;
            }
        }
        if (any) {
            sc = refine_finite(centre) ? centre : ninf;
            sb = bv;
        }
    }
    const int a = bi / (NS * NS) - A, sy = (bi / NS) % NS - S, sx = bi % NS - S;
    // an index that is 0 leaves its part of the pose bit for bit
    theta_out[i] = a == 0 ? th : add_rn(th, mul_rn((float)a, dtheta));
    dx_out[2 * (size_t)i] = sx == 0 ? d0 : add_rn(d0, div_rn(div_rn((float)(2 * sx), (float)(n - 1)), t_scale));
    dx_out[2 * (size_t)i + 1] = sy == 0 ? d1 : add_rn(d1, div_rn(div_rn((float)(-2 * sy), (float)(n - 1)), t_scale));
    score[2 * (size_t)i] = sc;
    score[2 * (size_t)i + 1] = sb;
    best[3 * (size_t)i] = a;
    best[3 * (size_t)i + 1] = sy;
    best[3 * (size_t)i + 2] = sx;
}

}  // namespace tvae_cluster
