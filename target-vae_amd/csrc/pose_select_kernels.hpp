// The selection of a hard pose search from its tables (libtvae_cluster.so): the arg-max of num / sqrt(pp yy) over the
// (slot, angle, shift) candidates of every image, with the template power pp given per candidate or per angle alone -- the
// form tvae_template_ctf_power writes, which does not depend on the shift.  include/tvae_cluster.h states the definition;
// with pp per candidate the outputs are those of classify_select_kernel bit for bit: the score, the finite test and the pose
// update are the device functions of refine_device.hpp.  Included by abi_pose_select.hip only.
//
// pose_select_kernel   a wavefront = one image, four images per workgroup of 256.  The lanes stride over the flat candidates
//                      of a slot, e = lane, lane + 64, ...: the loads of num (and of pp per candidate) are contiguous, pp per
//                      angle is one word for a run of NS^2 candidates.  A lane keeps its best as (score, key), key = -1 for
//                      the centre and the flat index otherwise, so that "greater score, then lower key" IS the rule of
//                      refine_select_candidate: the centre before every other equal maximum, then the lowest index.  That
//                      order is total, so the butterfly of six xor-shuffles leaves the same winner in every lane whatever
//                      the order of the comparisons.  The state across slots is uniform over the wave; lane 0 writes.
// No LDS, no atomics, no barrier; an image's outputs depend on its rows of the inputs only.
#pragma once
#include <hip/hip_runtime.h>

#include "refine_device.hpp"

// (fp contract stays off, as refine_device.hpp states it; said again so that this file does not lean on the include order)
#pragma clang fp contract(off)

namespace tvae_cluster {

constexpr int SELECT_WAVE = 64;                               // lanes of an image
constexpr int SELECT_IMAGES = REFINE_TILE / SELECT_WAVE;      // images of a workgroup
constexpr int SELECT_NONE = 0x7fffffff;                       // the key of "no finite candidate yet"

// (v, key) replaces (bv, bk): a strictly greater score, or the same score under a lower key
__device__ __forceinline__ bool select_better(float v, int key, float bv, int bk) { return v > bv || (v == bv && key < bk); }

// grid = ceil(N / 4).  cand [N][M]; num [N][M][NA][NS][NS]; pp the same (per_shift) or [N][M][NA]; yy [N]; cls_out [N],
// best [N][4] = (m, a, sy, sx), theta_out [N], dx_out [N][2], score [N][M][2]
__global__ __launch_bounds__(REFINE_TILE) void pose_select_kernel(
    const float* __restrict__ theta, const float* __restrict__ dx, const int* __restrict__ cand,
    const float* __restrict__ num, const float* __restrict__ pp, const float* __restrict__ yy, int* __restrict__ cls_out,
    int* __restrict__ best, float* __restrict__ theta_out, float* __restrict__ dx_out, float* __restrict__ score, int N, int n,
    int K, int M, int A, int S, int per_shift, float t_scale, float dtheta) {
    const int lane = threadIdx.x & (SELECT_WAVE - 1);
    const int i = blockIdx.x * SELECT_IMAGES + (threadIdx.x / SELECT_WAVE);
    if (i >= N) return;                                       // (uniform over the wave; the kernel has no barrier)
    const int NS = 2 * S + 1, NS2 = NS * NS, NA = 2 * A + 1, cnd = NA * NS2;
    const int ci = (A * NS + S) * NS + S;                     // the centre
    const int* __restrict__ row = cand + (size_t)i * M;
    const float y = yy[i];
    const float ninf = -__builtin_inff();
    // the angle of candidate e = lane + 64 j without a division per candidate: (a, r) = (e / NS2, e % NS2) moves by (qa, qr);
    // `a` is read only when the power is per angle (per_shift == 0) and carried along otherwise
    const int a0 = lane / NS2, r0 = lane - a0 * NS2, qa = SELECT_WAVE / NS2, qr = SELECT_WAVE - qa * NS2;
    int wm = -1, wbi = ci;                                    // the winning slot (none yet) and its candidate (the centre)
    float wsb = 0.f;
    for (int m = 0; m < M; ++m) {
        const int k = row[m];
        float sc = 0.f, sb = 0.f;
        if (k >= 0 && k < K) {                                // (uniform over the wave)
            const size_t slot = (size_t)i * M + m;
            const float* __restrict__ nu = num + slot * cnd;
            const float* __restrict__ pr = pp + slot * (per_shift ? cnd : NA);
            float bv = ninf, cv = ninf;                       // this lane's best, and the centre score where it owns the centre
            int bk = SELECT_NONE;
            int a = a0, r = r0;
            for (int e = lane; e < cnd; e += SELECT_WAVE) {
                const float v = refine_score(nu[e], pr[per_shift ? e : a], y);
                if (refine_finite(v)) {
                    const int key = e == ci ? -1 : e;
                    if (e == ci) cv = v;
                    if (select_better(v, key, bv, bk)) {
                        bv = v;
                        bk = key;
                    }
                }
                a += qa;
                r += qr;
                if (r >= NS2) {
                    r -= NS2;
                    ++a;
                }
            }
#pragma unroll
            for (int off = SELECT_WAVE / 2; off > 0; off >>= 1) {
                const float ov = __shfl_xor(bv, off, SELECT_WAVE);
                const int ok = __shfl_xor(bk, off, SELECT_WAVE);
                if (select_better(ov, ok, bv, bk)) {
                    bv = ov;
                    bk = ok;
                }
            }
            cv = __shfl(cv, ci & (SELECT_WAVE - 1), SELECT_WAVE);
            int bi = ci;
            if (bk != SELECT_NONE) {                          // something is finite
                sc = cv;
                sb = bv;
                bi = bk < 0 ? ci : bk;
            }
            if (wm < 0 || sb > wsb) {                         // ties stay with the lower slot
                wm = m;
                wbi = bi;
                wsb = sb;
            }
        }
        if (lane == 0) {
            score[2 * ((size_t)i * M + m)] = sc;
            score[2 * ((size_t)i * M + m) + 1] = sb;
        }
    }
    if (lane != 0) return;
    const int a = wbi / NS2 - A, sy = (wbi / NS) % NS - S, sx = wbi % NS - S;
    refine_write_pose(theta_out, dx_out, i, theta[i], dx[2 * (size_t)i], dx[2 * (size_t)i + 1], a, sy, sx, n, t_scale, dtheta);
    cls_out[i] = row[wm < 0 ? 0 : wm];
    best[4 * (size_t)i] = wm < 0 ? 0 : wm;
    best[4 * (size_t)i + 1] = a;
    best[4 * (size_t)i + 2] = sy;
    best[4 * (size_t)i + 3] = sx;
}

}  // namespace tvae_cluster
