// Eigenimages of the aligned classes (libtvae_cluster.so): the class covariance applied to a block of J vectors per class
// without ever writing the aligned stack.  With d_q the masked residual of position q of `order` against the average of its
// class (include/tvae_cluster.h states it: d = m * (a - mean), a the bilinear sample of align_sample),
//     project      coef[q][j] = <d_q, V[k][j]>,  norm2[q] = <d_q, d_q>
//     backproject  W[k][j]    = sum over the valid positions q of class k of coef[q][j] d_q
// so that backproject(project(V)) = R^T R V, R the matrix whose rows are the residuals of the class.
//
// eigen_prep_kernel         workgroup 0 cleans seg exactly as avg_seg_kernel does (running maximum, clamped to [0, N]); the
//                           workgroups behind it write the mask m[n][n] into the workspace, ONCE per call and not per sample.
// eigen_project_kernel<JT>  a workgroup = EIGEN_GROUP consecutive positions of `order`, all pixels and channels.  Thread t takes
//                           the pixels t, t + 256, ... of every channel in turn (the order of refine_sum_squares): per position
//                           one fp32 FMA chain per component and one for the norm, then the fixed binary tree over the 256
//                           threads in LDS.  The J values of V at a pixel sit in registers and serve every position of the group
//                           that belongs to the same class (`order` is sorted by class: that is all of them except at a class
//                           boundary, where they are loaded again) -- the grouping changes what is loaded, never a chain.
//                           Neighbouring workgroups read the same block V[k] (J C n n floats, 512 KB at 128 x 128 and J = 8):
//                           it stays in the L2 of every XCD while the class lasts.
// eigen_accum_kernel<JT>    a workgroup = 256 pixels x one channel x one chunk of EIGEN_CHUNK members, as avg_accum_kernel: one
//                           sample per member and pixel shared by the J chains acc[j] = fma(coef[q][j], d, acc[j]) in ascending
//                           position; the members' poses and coefficients sit in LDS and are read as broadcasts.
// eigen_reduce_kernel       a thread = an element of W[k][j][ch]: the class's slots in ascending order in fp64, rounded once.
// JT is J rounded up to 1, 2, 4, 8 or 16: the accumulators are registers with constant indices (no scratch); the components
// j >= J are never loaded, stored or reduced.
// Chunks and slots as in align_kernels.hpp with EIGEN_CHUNK for AVG_CHUNK: chunk c of class k owns the slot
// floor(s_k / EIGEN_CHUNK) + k + c.  No float atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include "cluster_common.hpp"

namespace tvae_cluster {

constexpr int EIGEN_TILE = 256;          // threads per workgroup = pixels per tile
constexpr int EIGEN_CHUNK = 128;         // members of a class per partial sum (J planes per slot: 4 x AVG_CHUNK keeps them few)
constexpr int EIGEN_GROUP = 4;           // positions of `order` per workgroup of the projection
constexpr int EIGEN_J_MAX = TVAE_EIGEN_MAX_COMPONENTS;
constexpr int EIGEN_C_MAX = 1024;        // channels (ALIGN_C_MAX)

static inline int eigen_tiles(int n) { return (n * n + EIGEN_TILE - 1) / EIGEN_TILE; }
static inline long eigen_slots(int N, int K) { return (long)N / EIGEN_CHUNK + K; }

// grid = 1 + tiles.  clean[k] = min(max(0, seg[0], ..., seg[k]), N); mask[n][n]: the mask of tvae_class_frc at the canonical
// pixel, fp64 rounded to fp32 once, 1 everywhere for radius <= 0
__global__ __launch_bounds__(EIGEN_TILE) void eigen_prep_kernel(const int* __restrict__ seg, int* __restrict__ clean, int K,
                                                                int N, float* __restrict__ mask, int n, float radius,
                                                                float edge) {
    __shared__ int part[EIGEN_TILE];
    if (blockIdx.x > 0) {
        const int p = (blockIdx.x - 1) * EIGEN_TILE + threadIdx.x;
        if (p >= n * n) return;
        float m = 1.f;
        if (radius > 0.f) {
            const double c = 0.5 * (double)(n - 1);
            const double di = (double)(p / n) - c, dj = (double)(p % n) - c;
            m = soft_mask(sqrt(di * di + dj * dj), radius, edge);
        }
        mask[p] = m;
        return;
    }
    const int len = K + 1;
    const int per = (len + EIGEN_TILE - 1) / EIGEN_TILE;
    const int lo = min((int)threadIdx.x * per, len), hi = min(lo + per, len);
    int m = 0;
    for (int k = lo; k < hi; ++k) m = max(m, seg[k]);
    part[threadIdx.x] = m;
    __syncthreads();
    int run = 0;                                              // maximum of everything in front of this thread's share
    for (int t = 0; t < (int)threadIdx.x; ++t) run = max(run, part[t]);
    for (int k = lo; k < hi; ++k) {
        run = max(run, seg[k]);
        clean[k] = min(run, N);
    }
}

__device__ __forceinline__ AlignPose eigen_pose(const float* __restrict__ theta, const float* __restrict__ dx, int id,
                                                float t_scale) {
    AlignPose q;
    const float th = theta[id];
    q.c = cosf(th);
    q.s = sinf(th);
    q.tx = t_scale * dx[2 * (long)id];
    q.ty = t_scale * dx[2 * (long)id + 1];
    return q;
}

// grid = ceil(N / EIGEN_GROUP).  coef[N][J], norm2[N] (or NULL): rows by position in `order`
template <int JT>
__global__ __launch_bounds__(EIGEN_TILE) void eigen_project_kernel(
    const float* __restrict__ Y, const float* __restrict__ theta, const float* __restrict__ dx,
    const int* __restrict__ order, const int* __restrict__ clean, const float* __restrict__ mean,
    const float* __restrict__ V, const float* __restrict__ mask, float* __restrict__ coef, float* __restrict__ norm2, int N,
    int C, int n, int K, int J, float t_scale) {
    __shared__ AlignPose pose[EIGEN_GROUP];
    __shared__ int member[EIGEN_GROUP], cls[EIGEN_GROUP];
    __shared__ float red[(JT + 1) * EIGEN_TILE];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * EIGEN_GROUP;
    if (tid < EIGEN_GROUP) {
        const int q = q0 + tid;
        int id = -1, k = 0;
        if (q < N && q >= clean[0] && q < clean[K]) {
            int lo = 0, hi = K - 1;                           // the largest k with clean[k] <= q: q < clean[k + 1] follows
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (clean[mid] <= q) lo = mid; else hi = mid - 1;
            }
            k = lo;
            id = order[q];
            if (id < 0 || id >= N) id = -1;
        }
        AlignPose ps = {0.f, 0.f, 0.f, 0.f};
        if (id >= 0) ps = eigen_pose(theta, dx, id, t_scale);
        pose[tid] = ps;
        member[tid] = id;
        cls[tid] = k;
    }
    __syncthreads();
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const int npix = n * n;
    const size_t nn = (size_t)npix;
    float acc[EIGEN_GROUP][JT], nrm[EIGEN_GROUP];
#pragma unroll
    for (int g = 0; g < EIGEN_GROUP; ++g) {
        nrm[g] = 0.f;
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) acc[g][jj] = 0.f;
    }
    for (int ch = 0; ch < C; ++ch) {
        for (int e = tid; e < npix; e += EIGEN_TILE) {
            const int i = e / n, j = e - i * n;
            const float mk = mask[e];
            float v[JT];
            int cur = -1;                                     // the class whose V is in v: uniform over the workgroup
#pragma unroll
            for (int g = 0; g < EIGEN_GROUP; ++g) {
                const int id = member[g];
                if (id < 0) continue;
                const int k = cls[g];
                if (k != cur) {
                    cur = k;
#pragma unroll
                    for (int jj = 0; jj < JT; ++jj)
                        v[jj] = jj < J ? V[(((size_t)k * J + jj) * C + ch) * nn + e] : 0.f;
                }
                const float a = align_sample(Y + ((size_t)id * C + ch) * nn, n, i, j, step, half, pose[g], true);
                const float r = a - mean[((size_t)k * C + ch) * nn + e];
                const float d = mk * r;
                nrm[g] = fmaf(d, d, nrm[g]);
#pragma unroll
                for (int jj = 0; jj < JT; ++jj) acc[g][jj] = fmaf(d, v[jj], acc[g][jj]);
            }
        }
    }
    // per position: J + 1 sums, each through the tree  red[t] += red[t + w], w = 128, 64, ..., 1
    const int outs = J + 1;
#pragma unroll
    for (int g = 0; g < EIGEN_GROUP; ++g) {
        const int q = q0 + g;
        if (q >= N) break;                                    // (uniform)
        if (member[g] < 0) {
            if (tid < J) coef[(size_t)q * J + tid] = 0.f;
            if (tid == 0 && norm2) norm2[q] = 0.f;
            continue;
        }
#pragma unroll
        for (int jj = 0; jj < JT; ++jj)
            if (jj < J) red[jj * EIGEN_TILE + tid] = acc[g][jj];
        red[J * EIGEN_TILE + tid] = nrm[g];
        __syncthreads();
        for (int w = EIGEN_TILE / 2, sh = 7; w > 0; w >>= 1, --sh) {
            for (int it = tid; it < outs * w; it += EIGEN_TILE) {
                const int o = it >> sh, t = it & (w - 1);
                red[o * EIGEN_TILE + t] += red[o * EIGEN_TILE + t + w];
            }
            __syncthreads();
        }
        if (tid < J) coef[(size_t)q * J + tid] = red[tid * EIGEN_TILE];
        if (tid == 0 && norm2) norm2[q] = red[J * EIGEN_TILE];
        __syncthreads();
    }
}

// grid = slots * C * tiles (tile fastest, then channel).  part[slots][J][C][n][n], cnt[slots] (written by tile 0 of channel 0)
template <int JT>
__global__ __launch_bounds__(EIGEN_TILE) void eigen_accum_kernel(
    const float* __restrict__ Y, const float* __restrict__ theta, const float* __restrict__ dx,
    const int* __restrict__ order, const int* __restrict__ clean, const float* __restrict__ mean,
    const float* __restrict__ coef, const float* __restrict__ mask, float* __restrict__ part, int* __restrict__ cnt, int N,
    int C, int n, int K, int J, int tiles, float t_scale) {
    __shared__ AlignPose pose[EIGEN_CHUNK];
    __shared__ int member[EIGEN_CHUNK];
    __shared__ float cf[EIGEN_CHUNK * JT];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles;
    const long rest = blockIdx.x / tiles;
    const int ch = (int)(rest % C);
    const int slot = (int)(rest / C);
    // The return depends on blockIdx and `clean` alone: uniform, and in front of every barrier.
    ChunkSpan span;
    if (!chunk_of_slot(clean, K, slot, EIGEN_CHUNK, span)) return;       // a slot that no chunk owns
    const int k = span.k, first = span.first, members = span.members;
    if (tid < EIGEN_CHUNK) {
        int id = -1;
        if (tid < members) {
            id = order[first + tid];
            if (id < 0 || id >= N) id = -1;
        }
        AlignPose ps = {0.f, 0.f, 0.f, 0.f};
        if (id >= 0) ps = eigen_pose(theta, dx, id, t_scale);
        pose[tid] = ps;
        member[tid] = id;
    }
    for (int it = tid; it < members * JT; it += EIGEN_TILE) {
        const int m = it / JT, jj = it - m * JT;
        cf[it] = jj < J ? coef[(size_t)(first + m) * J + jj] : 0.f;
    }
    __syncthreads();
    if (tile == 0 && ch == 0 && tid == 0) {
        int v = 0;
        for (int m = 0; m < members; ++m) v += member[m] >= 0;
        cnt[slot] = v;
    }
    const int p = tile * EIGEN_TILE + tid;
    if (p >= n * n) return;
    const int i = p / n, j = p - i * n;
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const size_t nn = (size_t)n * n;
    const float mk = mask[p];
    const float mu = mean[((size_t)k * C + ch) * nn + p];
    float acc[JT];
#pragma unroll
    for (int jj = 0; jj < JT; ++jj) acc[jj] = 0.f;
#pragma unroll 2
    for (int m = 0; m < members; ++m) {
        const int id = member[m];
        if (id < 0) continue;                                 // (uniform) a skipped entry adds nothing
        const float a = align_sample(Y + ((size_t)id * C + ch) * nn, n, i, j, step, half, pose[m], true);
        const float r = a - mu;
        const float d = mk * r;
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) acc[jj] = fmaf(cf[m * JT + jj], d, acc[jj]);
    }
#pragma unroll
    for (int jj = 0; jj < JT; ++jj)
        if (jj < J) part[(((size_t)slot * J + jj) * C + ch) * nn + p] = acc[jj];
}

// grid = K * J * C * tiles (tile fastest).  W[K][J][C][n][n], counts[K] (written by tile 0 of component 0, channel 0)
__global__ __launch_bounds__(EIGEN_TILE) void eigen_reduce_kernel(const float* __restrict__ part,
                                                                  const int* __restrict__ cnt,
                                                                  const int* __restrict__ clean, float* __restrict__ W,
                                                                  int* __restrict__ counts, int C, int n, int J, int tiles) {
    const int tile = blockIdx.x % tiles;
    const long plane = blockIdx.x / tiles;                    // (class * J + component) * C + channel
    const int ch = (int)(plane % C);
    const long kj = plane / C;
    const int jj = (int)(kj % J), k = (int)(kj / J);
    const int sk = clean[k], ek = clean[k + 1];
    const int chunks = (ek - sk + EIGEN_CHUNK - 1) / EIGEN_CHUNK;
    const int slot0 = sk / EIGEN_CHUNK + k;
    if (tile == 0 && jj == 0 && ch == 0 && threadIdx.x == 0) {
        int v = 0;
        for (int c = 0; c < chunks; ++c) v += cnt[slot0 + c];
        counts[k] = v;
    }
    const int p = tile * EIGEN_TILE + threadIdx.x;
    if (p >= n * n) return;
    const size_t nn = (size_t)n * n;
    double sum = 0.0;
    for (int c = 0; c < chunks; ++c) sum += (double)part[(((size_t)(slot0 + c) * J + jj) * C + ch) * nn + p];
    W[(size_t)plane * nn + p] = (float)sum;
}

}  // namespace tvae_cluster
