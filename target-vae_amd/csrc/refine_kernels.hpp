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

#include "refine_device.hpp"

// (fp contract stays off, as refine_device.hpp states it; said again so that this file does not lean on the include order)
#pragma clang fp contract(off)

namespace tvae_cluster {

// floats of LDS: the image plane and the template (the partial sums [NS][G][NS] take their place at the end), R2 and the 256
// partials of yy
static inline size_t refine_lds_floats(int n, int S) {
    const int NS = 2 * S + 1, ne = n + 2 * S;
    const size_t planes = (size_t)n * refine_stride(n) + (size_t)ne * refine_stride(ne);
    const size_t parts = (size_t)NS * refine_groups(n, NS) * NS;
    return (planes > parts ? planes : parts) + (size_t)ne * NS + REFINE_TILE;
}

// grid = N * NA (angle fastest).  num, pp [N][NA][NS][NS], yy [N].  The steps are the functions of refine_device.hpp.
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

    const RefinePose pose = refine_angle_pose(theta, dx, img, ai, A, t_scale, dtheta);
    const size_t nn = (size_t)n * n;

    const bool worker = tid < NS * G;
    const int syi = tid / G, g = tid - syi * G;               // the row shift sy = syi - S and the row group of this thread
    float acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.f;

    for (int ch = 0; ch < C; ++ch) {
        if (ch > 0) __syncthreads();                          // the previous channel's planes are still being read
        refine_load_plane(ys, Y + ((size_t)img * C + ch) * nn, n, ystride, tid);
        refine_build_template<S>(ts, ref + ((size_t)k * C + ch) * nn, n, pose, mask_radius, mask_edge, tid);
        __syncthreads();
        if (worker) refine_correlate<S>(ts, ys, acc, n, G, syi, g);
        refine_row_squares<S>(ts, r2s, n, ch == 0, tid);
    }
    refine_store_sums<S>(pn, r2s, acc, numo, ppo, n, G, worker, syi, g, tid);
    if (ai == 0) refine_sum_squares(Y + (size_t)img * C * nn, C, n, red, yy + img, tid);      // (uniform)
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
    if (k >= 0 && k < K) bi = refine_select_candidate(num + (size_t)i * cand, pp + (size_t)i * cand, yy[i], A, S, sc, sb);
    const int a = bi / (NS * NS) - A, sy = (bi / NS) % NS - S, sx = bi % NS - S;
    refine_write_pose(theta_out, dx_out, i, th, d0, d1, a, sy, sx, n, t_scale, dtheta);
    score[2 * (size_t)i] = sc;
    score[2 * (size_t)i + 1] = sb;
    best[3 * (size_t)i] = a;
    best[3 * (size_t)i + 1] = sy;
    best[3 * (size_t)i + 2] = sx;
}

}  // namespace tvae_cluster
