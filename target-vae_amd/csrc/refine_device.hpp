// The device functions of the pose search against a reference (libtvae_cluster.so): what one workgroup does for one
// (image, angle, reference) -- the extended template, the sliding-ring correlation, the separable sum of T^2 -- and what one
// thread does to pick an image's candidate.  refine_kernels.hpp (one reference per image) and classify_kernels.hpp (M
// candidate references per image) call them, so a slot of tvae_pose_classify is tvae_pose_refine bit for bit by construction.
// The host part states the shape range of a pose search once, for abi_refine.hip, abi_classify.hip, abi_ml2d.hip and
// abi_polish.hip, and dispatches over the shift radius.
// Host and device code and NO __global__ function (cluster_common.hpp says why): the kernel headers of the pose searches
// include this one.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cluster_common.hpp"

// The definition rounds every product and sum on its own (theta + a dtheta above all: the refined angle is compared bit for
// bit).  The runtime's __fmul_rn and __fadd_rn are plain operators that the compiler may still fuse after inlining, so the
// operations of this file and of the two kernel headers are its own, defined under contract(off): every fused multiply-add
// below is an fmaf.
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

// ---- host: the range of a pose search, its candidates per (image, reference), the dispatch over the shift radius ------------
static inline bool refine_shape_ok(long N, long C, long n, long A, long S) {
    return N >= 1 && N <= PLANES_MAX && C >= 1 && C <= REFINE_C_MAX && n >= 2 && n <= REFINE_SIDE_MAX && A >= 0 &&
           A <= REFINE_A_MAX && S >= 0 && S <= REFINE_S_MAX;      // (N NA workgroups: at most 2^24 * 65 < 2^31)
}
static inline long refine_cand(int A, int S) { return (2L * A + 1) * (2 * S + 1) * (2 * S + 1); }

// launch(std::integral_constant<int, S>) for the S in 0 .. REFINE_S_MAX that was asked for: the kernels take S as a template
// argument.  -> what `launch` returns, or hipErrorInvalidValue for another S.
template <class Launch>
static inline int refine_by_shift(int S, Launch&& launch) {
    switch (S) {
        case 0: return launch(std::integral_constant<int, 0>{});
        case 1: return launch(std::integral_constant<int, 1>{});
        case 2: return launch(std::integral_constant<int, 2>{});
        case 3: return launch(std::integral_constant<int, 3>{});
        case 4: return launch(std::integral_constant<int, 4>{});
        case 5: return launch(std::integral_constant<int, 5>{});
        case 6: return launch(std::integral_constant<int, 6>{});
        case 7: return launch(std::integral_constant<int, 7>{});
        case 8: return launch(std::integral_constant<int, 8>{});
    }
    return (int)hipErrorInvalidValue;
}

// ---- device -----------------------------------------------------------------------------------------------------------------
// row stride of a plane of `side` columns in LDS: odd
__host__ __device__ static inline int refine_stride(int side) { return side | 1; }

// G: the row groups of a row shift.  At most REFINE_TILE / NS (one thread per (sy, g)); as few rows per group as that
// allows, and then no more groups than those rows need.  1 <= G <= n.
__host__ __device__ static inline int refine_groups(int n, int NS) {
    const int cap = REFINE_TILE / NS;
    const int rows = (n + cap - 1) / cap;
    return (n + rows - 1) / rows;
}

// the pose of one angle of an image: every operation rounded to fp32 on its own
struct RefinePose {
    float c, s, tx, ty;
};
__device__ __forceinline__ RefinePose refine_angle_pose(const float* __restrict__ theta, const float* __restrict__ dx,
                                                        int img, int ai, int A, float t_scale, float dtheta) {
    const float th = add_rn(theta[img], mul_rn((float)(ai - A), dtheta));
    RefinePose p;
    p.c = cosf(th);
    p.s = sinf(th);
    p.tx = mul_rn(t_scale, dx[2 * (size_t)img]);
    p.ty = mul_rn(t_scale, dx[2 * (size_t)img + 1]);
    return p;
}

// Where the pixel at column q and row r of the image frame (q, r may lie outside it: the extended template) reads the
// reference under the pose p: (u0, u1) in coordinate units and (col, row) in pixels of the reference.  THE position arithmetic
// of the pose searches: refine_build_template and polish_moments_kernel both call it, so the template of the polish is that of
// refinement at A = 0, S = 0 bit for bit by construction.
struct RefinePosition {
    float u0, u1, col, row;
};
__device__ __forceinline__ RefinePosition refine_position(int q, int r, float step, float half, RefinePose p) {
    const float x0 = fmaf((float)q, step, -1.f);
    const float x1 = fmaf(-(float)r, step, 1.f);
    const float v0 = x0 - p.tx, v1 = x1 - p.ty;
    RefinePosition at;
    at.u0 = fmaf(v0, p.c, -mul_rn(v1, p.s));
    at.u1 = fmaf(v0, p.s, mul_rn(v1, p.c));
    at.col = mul_rn(at.u0 + 1.f, half);
    at.row = mul_rn(1.f - at.u1, half);
    return at;
}

// ys [n][ystride] = the plane Yp [n][n]
__device__ __forceinline__ void refine_load_plane(float* __restrict__ ys, const float* __restrict__ Yp, int n, int ystride,
                                                  int tid) {
    for (int e = tid; e < n * n; e += REFINE_TILE) {
        const int r = e / n, q = e - r * n;
        ys[r * ystride + q] = Yp[e];
    }
}

// ts [ne][tstride] = the template of the plane Rp [n][n] at the pose p on the grid extended by S pixels
template <int S>
__device__ __forceinline__ void refine_build_template(float* __restrict__ ts, const float* __restrict__ Rp, int n,
                                                      RefinePose p, float mask_radius, float mask_edge, int tid) {
    const int ne = n + 2 * S, tstride = refine_stride(ne);
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const bool masked = mask_radius > 0.f;
    for (int e = tid; e < ne * ne; e += REFINE_TILE) {
        const int re = e / ne, qe = e - re * ne;
        const RefinePosition at = refine_position(qe - S, re - S, step, half, p);
        float v = bilinear_zero_border(Rp, n, at.col, at.row, true);
        if (masked) {
            // out of frame (NaN and +-inf among it) stays an exact 0 whatever the mask would be there
            const bool in = inside_frame(at.col, at.row, n);
            const double d = sqrt((double)at.u0 * (double)at.u0 + (double)at.u1 * (double)at.u1) * (0.5 * (double)(n - 1));
            v = in ? mul_rn(soft_mask(d, mask_radius, mask_edge), v) : 0.f;
        }
        ts[re * tstride + qe] = v;
    }
}

// num: thread (syi, g) adds the rows r = g, g + G, ... of one channel to its NS sums over sx; along a row the NS template
// values under the window slide through a register ring
template <int S>
__device__ __forceinline__ void refine_correlate(const float* __restrict__ ts, const float* __restrict__ ys,
                                                 float (&acc)[2 * S + 1], int n, int G, int syi, int g) {
    constexpr int NS = 2 * S + 1;
    const int ne = n + 2 * S, ystride = refine_stride(n), tstride = refine_stride(ne);
    for (int r = g; r < n; r += G) {
        const float* __restrict__ trow = ts + (r + 2 * S - syi) * tstride;   // T_a[r - sy], extended row index
        const float* __restrict__ yrow = ys + r * ystride;
        float ring[NS];                                       // T[q + j] at slot (q + j) % NS
#pragma unroll
        for (int j = 0; j < NS; ++j) ring[j] = trow[j];
        for (int q0 = 0; q0 < n; q0 += NS) {
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const int q = q0 + u;
                if (q < n) {                                  // (uniform)
                    const float y = yrow[q];
#pragma unroll
                    for (int sxi = 0; sxi < NS; ++sxi)        // P(r, q) = T[r - sy][q - sx]: column q + 2S - sxi
                        acc[sxi] = fmaf(ring[(u + 2 * S - sxi) % NS], y, acc[sxi]);
                    if (q + NS < ne) ring[u] = trow[q + NS];
                }
            }
        }
    }
}

// R2 [ne][NS]: the sum of T^2 over the n columns of the window, carried on through the channels (`first`: the chain
// starts); the same thread owns R2[e] in every channel
template <int S>
__device__ __forceinline__ void refine_row_squares(const float* __restrict__ ts, float* __restrict__ r2s, int n, bool first,
                                                   int tid) {
    constexpr int NS = 2 * S + 1;
    const int ne = n + 2 * S, tstride = refine_stride(ne);
    for (int e = tid; e < ne * NS; e += REFINE_TILE) {
        const int re = e / NS, sxi = e - re * NS;
        const float* __restrict__ trow = ts + re * tstride + (2 * S - sxi);
        float a = first ? 0.f : r2s[e];
        for (int q = 0; q < n; ++q) {
            const float v = trow[q];
            a = fmaf(v, v, a);
        }
        r2s[e] = a;
    }
}

// The end of an (image, angle, reference): the G partial sums of a candidate through pn [NS][G][NS] in ascending g into numo,
// and R2 over the window's rows into ppo [NS][NS].  Every thread of the workgroup calls it; pn may take the place of planes
// that every thread is done with when the call begins (it starts with a barrier).
template <int S>
__device__ __forceinline__ void refine_store_sums(float* __restrict__ pn, const float* __restrict__ r2s,
                                                  const float (&acc)[2 * S + 1], float* __restrict__ numo,
                                                  float* __restrict__ ppo, int n, int G, bool worker, int syi, int g, int tid) {
    constexpr int NS = 2 * S + 1;
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
}

// yy of an image Yi [C][n][n] -> *yyo: thread t adds the pixels t, t + 256, ... of every channel in turn, then a binary tree
// over red [REFINE_TILE].  Every thread of the workgroup calls it.
__device__ __forceinline__ void refine_sum_squares(const float* __restrict__ Yi, int C, int n, float* __restrict__ red,
                                                   float* __restrict__ yyo, int tid) {
    const size_t nn = (size_t)n * n;
    float a = 0.f;
    for (int ch = 0; ch < C; ++ch) {
        const float* __restrict__ Yp = Yi + ch * nn;
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
    if (tid == 0) *yyo = red[0];
}

__device__ __forceinline__ bool refine_finite(float x) { return x - x == 0.f; }

// score of one candidate from its three sums: fp64, rounded to fp32 once; exactly 0 where pp or yy is 0
__device__ __forceinline__ float refine_score(float nu, float p, float y) {
    if (p == 0.f || y == 0.f) return 0.f;
    return (float)__ddiv_rn((double)nu, __dsqrt_rn(__dmul_rn((double)p, (double)y)));   // each correctly rounded
}

// The selection rule over the NA NS^2 candidates of one (image, reference), nu and p its rows of the tables: -> the flat index
// of the best candidate, the centre if nothing is finite, and (sc, sb) = (centre, best), (0, 0) if nothing is finite.
__device__ __forceinline__ int refine_select_candidate(const float* __restrict__ nu, const float* __restrict__ p, float y,
                                                       int A, int S, float& sc, float& sb) {
    const int NS = 2 * S + 1, cand = (2 * A + 1) * NS * NS;
    int bi = (A * NS + S) * NS + S;                           // the centre
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
    sc = sb = 0.f;
    if (any) {
        sc = refine_finite(centre) ? centre : ninf;
        sb = bv;
    }
    return bi;
}

// the pose of the candidate (a, sy, sx): an index that is 0 leaves its part of the pose bit for bit
__device__ __forceinline__ void refine_write_pose(float* __restrict__ theta_out, float* __restrict__ dx_out, int i, float th,
                                                  float d0, float d1, int a, int sy, int sx, int n, float t_scale,
                                                  float dtheta) {
    theta_out[i] = a == 0 ? th : add_rn(th, mul_rn((float)a, dtheta));
    dx_out[2 * (size_t)i] = sx == 0 ? d0 : add_rn(d0, div_rn(div_rn((float)(2 * sx), (float)(n - 1)), t_scale));
    dx_out[2 * (size_t)i + 1] = sy == 0 ? d1 : add_rn(d1, div_rn(div_rn((float)(-2 * sy), (float)(n - 1)), t_scale));
}

}  // namespace tvae_cluster
