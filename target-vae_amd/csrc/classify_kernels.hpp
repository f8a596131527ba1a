// Reassignment against the class averages (libtvae_cluster.so): the pose search of refine_kernels.hpp against M candidate
// references per image instead of one, and the choice among them.  A slot of tvae_pose_classify is tvae_pose_refine with
// cls = cand[:, m] bit for bit: both kernels call the device functions of refine_device.hpp, and nothing of a slot's chains
// depends on the other slots.  include/tvae_cluster.h states the definition.  Included by abi_classify.hip only.
//
// classify_corr_kernel<S>  a workgroup = one (image, angle), 256 threads, looping over the M slots.  What does not depend on
//                          the slot is formed once per workgroup: the angle's cos and sin and t dx, the validity of the
//                          row of candidates, and for C = 1 the image plane in LDS (with C > 1 a slot's chains run through
//                          the channels, so the plane of a channel is loaded again for every slot, as M calls of
//                          refine_corr_kernel would).  yy is formed once per image, by the workgroup of the first angle.
//                          A skipped slot costs its store of zeros.  LDS: [ys | ts or the partial sums | R2 | red]; the
//                          partial sums take the place of the template alone, because the image plane stays.  That is the
//                          footprint of refine_corr_kernel<S> wherever the two planes outweigh the partial sums, n = 128
//                          among it.
// classify_select_kernel   a thread = an image: the rule of refine_select_kernel per slot, then the rule across slots
//                          (ascending m, replaced only by a strictly greater best score), and the pose of the winner.
// No atomics; an image's outputs depend on (n, S, C, A), its row of candidates and the references it names only.
#pragma once
#include <hip/hip_runtime.h>

#include "refine_device.hpp"

// (fp contract stays off, as refine_device.hpp states it; said again so that this file does not lean on the include order)
#pragma clang fp contract(off)

namespace tvae_cluster {

constexpr int CLASSIFY_M_MAX = TVAE_CLASSIFY_MAX_CANDIDATES;

// floats of LDS: the image plane, then the template or the partial sums [NS][G][NS], R2 and the 256 partials of yy
static inline size_t classify_lds_floats(int n, int S) {
    const int NS = 2 * S + 1, ne = n + 2 * S;
    const size_t tpl = (size_t)ne * refine_stride(ne), parts = (size_t)NS * refine_groups(n, NS) * NS;
    return (size_t)n * refine_stride(n) + (tpl > parts ? tpl : parts) + (size_t)ne * NS + REFINE_TILE;
}

// grid = N * NA (angle fastest).  cand [N][M]; num, pp [N][M][NA][NS][NS], yy [N]
template <int S>
__global__ __launch_bounds__(REFINE_TILE) void classify_corr_kernel(
    const float* __restrict__ Y, const float* __restrict__ theta, const float* __restrict__ dx,
    const int* __restrict__ cand, const float* __restrict__ ref, float* __restrict__ num, float* __restrict__ pp,
    float* __restrict__ yy, int C, int n, int K, int M, int A, float t_scale, float dtheta, float mask_radius,
    float mask_edge) {
    constexpr int NS = 2 * S + 1;
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int NA = 2 * A + 1;
    const int img = blockIdx.x / NA, ai = blockIdx.x - img * NA;
    const int* __restrict__ row = cand + (size_t)img * M;
    const int ne = n + 2 * S, ystride = refine_stride(n), tstride = refine_stride(ne);
    const int G = refine_groups(n, NS);
    float* __restrict__ ys = lds;                             // [n][ystride]
    float* __restrict__ ts = ys + n * ystride;                // [ne][tstride]
    float* __restrict__ pn = ts;                              // [NS][G][NS], once a slot's template is done with
    const size_t tpl = (size_t)ne * tstride, parts = (size_t)NS * G * NS;
    float* __restrict__ r2s = ts + (tpl > parts ? tpl : parts);          // [ne][NS]
    float* __restrict__ red = r2s + ne * NS;                  // [REFINE_TILE]

    // (M <= 64 < the workgroup: one candidate per thread)
    const int mine = tid < M ? row[tid] : -1;
    const bool any = __syncthreads_or(mine >= 0 && mine < K) != 0;
    const RefinePose pose = refine_angle_pose(theta, dx, img, ai, A, t_scale, dtheta);
    const size_t nn = (size_t)n * n;
    const float* __restrict__ Yi = Y + (size_t)img * C * nn;

    const bool worker = tid < NS * G;
    const int syi = tid / G, g = tid - syi * G;               // the row shift sy = syi - S and the row group of this thread
    bool loaded = false;                                      // C = 1: the image plane is in ys

    for (int m = 0; m < M; ++m) {
        float* __restrict__ numo = num + (((size_t)img * M + m) * NA + ai) * (NS * NS);
        float* __restrict__ ppo = pp + (((size_t)img * M + m) * NA + ai) * (NS * NS);
        const int k = row[m];
        if (k < 0 || k >= K) {                                // uniform over the workgroup
            for (int e = tid; e < NS * NS; e += REFINE_TILE) {
                numo[e] = 0.f;
                ppo[e] = 0.f;
            }
            continue;
        }
        float acc[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] = 0.f;
        for (int ch = 0; ch < C; ++ch) {
            __syncthreads();                                  // the planes and sums of the step before are still being read
            if (!loaded) refine_load_plane(ys, Yi + ch * nn, n, ystride, tid);
            loaded = C == 1;
            refine_build_template<S>(ts, ref + ((size_t)k * C + ch) * nn, n, pose, mask_radius, mask_edge, tid);
            __syncthreads();
            if (worker) refine_correlate<S>(ts, ys, acc, n, G, syi, g);
            refine_row_squares<S>(ts, r2s, n, ch == 0, tid);
        }
        refine_store_sums<S>(pn, r2s, acc, numo, ppo, n, G, worker, syi, g, tid);
    }
    if (ai == 0) {                                            // (uniform)
        if (any)
            refine_sum_squares(Yi, C, n, red, yy + img, tid);
        else if (tid == 0)
            yy[img] = 0.f;
    }
}

// grid = ceil(N / 256).  cls_out [N], best [N][4] = (m, a, sy, sx), theta_out [N], dx_out [N][2], score [N][M][2]
__global__ __launch_bounds__(REFINE_TILE) void classify_select_kernel(
    const float* __restrict__ theta, const float* __restrict__ dx, const int* __restrict__ cand,
    const float* __restrict__ num, const float* __restrict__ pp, const float* __restrict__ yy, int* __restrict__ cls_out,
    float* __restrict__ theta_out, float* __restrict__ dx_out, float* __restrict__ score, int* __restrict__ best, int N,
    int n, int K, int M, int A, int S, float t_scale, float dtheta) {
    const int i = blockIdx.x * REFINE_TILE + threadIdx.x;
    if (i >= N) return;
    const int NS = 2 * S + 1, NA = 2 * A + 1, cnd = NA * NS * NS;
    const float th = theta[i], d0 = dx[2 * (size_t)i], d1 = dx[2 * (size_t)i + 1];
    const int* __restrict__ row = cand + (size_t)i * M;
    const float y = yy[i];
    int wm = -1, wbi = (A * NS + S) * NS + S;                 // the winning slot (none yet) and its candidate (the centre)
    float wsb = 0.f;
    for (int m = 0; m < M; ++m) {
        const int k = row[m];
        float sc = 0.f, sb = 0.f;
        if (k >= 0 && k < K) {
            const size_t at = ((size_t)i * M + m) * cnd;
            const int bi = refine_select_candidate(num + at, pp + at, y, A, S, sc, sb);
            if (wm < 0 || sb > wsb) {                         // ties stay with the lower slot
                wm = m;
                wbi = bi;
                wsb = sb;
            }
        }
        score[2 * ((size_t)i * M + m)] = sc;
        score[2 * ((size_t)i * M + m) + 1] = sb;
    }
    const int a = wbi / (NS * NS) - A, sy = (wbi / NS) % NS - S, sx = wbi % NS - S;
    refine_write_pose(theta_out, dx_out, i, th, d0, d1, a, sy, sx, n, t_scale, dtheta);
    cls_out[i] = row[wm < 0 ? 0 : wm];
    best[4 * (size_t)i] = wm < 0 ? 0 : wm;
    best[4 * (size_t)i + 1] = a;
    best[4 * (size_t)i + 2] = sy;
    best[4 * (size_t)i + 3] = sx;
}

}  // namespace tvae_cluster
