// Aligned 2-D class averages (libtvae_cluster.so): every image of a stack resampled into the canonical frame with its
// predicted rotation and translation, and the per-class means of those images without ever writing them.
//
// The pose convention is the model's (train_*.py: a pixel at coordinate x shows canonical content at
// u = (x - t dx) R(theta), coordinates linspace(-1, 1, n) along columns and linspace(1, -1, n) along rows), so the aligned
// image at the canonical grid point u reads image i at x = u R(theta)^T + t dx:
//     x0 = u0 c + u1 s + t dx0,  x1 = -u0 s + u1 c + t dx1,  col = (x0 + 1) (n - 1) / 2,  row = (1 - x1) (n - 1) / 2
// bilinear over the taps floor and floor + 1 per axis, a tap outside [0, n - 1] is 0 (zero border: the sample is a
// continuous function of the position) and a position that is not inside (-1, n) on both axes gives exactly 0 -- the
// range is tested BEFORE the float -> int conversion and NaN fails it.
//
// align_stack_kernel    a thread = an output pixel of one (image, channel), a workgroup = 256 consecutive pixels.  cosf and
//                       sinf (the accurate ones) once per workgroup, through LDS.
// avg_seg_kernel        ONE workgroup turns seg[K + 1] into a monotone sequence within [0, N] (running maximum, clamped):
//                       whatever seg holds, the launches below follow the cleaned copy and stay inside `order`.
// avg_accum_kernel      a workgroup = 256 pixels x one channel x one CHUNK of a class: up to AVG_CHUNK members of the class
//                       in the order of `order`.  The members' poses (cosf / sinf once per (workgroup, member)) sit in LDS
//                       and are read as broadcasts; the taps are plain global gathers (neighbouring pixels read
//                       neighbouring source pixels, the lines come from L2), always issued on clamped in-bounds addresses
//                       and then selected, so that the member loop is branch-free and unrolls.  The fp32 sum over the
//                       chunk's members in ascending position goes to the chunk's slot of the workspace.
// avg_reduce_kernel     a thread = a pixel of avg[k][ch]: the class's slots in ascending order, divided by the number of
//                       members that were not skipped.
// Chunk c of class k covers the positions [s_k + c AVG_CHUNK, min(s_k + (c + 1) AVG_CHUNK, e_k)) of `order` and owns the
// slot floor(s_k / AVG_CHUNK) + k + c: slots of different classes never collide for a monotone seg, there are at most
// N / AVG_CHUNK + K of them, and the split of a class depends on its own length only.  No float atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include "cluster_common.hpp"         // AlignPose and align_sample: shared with the eigenimage kernels

namespace tvae_cluster {

constexpr int ALIGN_TILE = 256;          // pixels per workgroup = threads per workgroup
constexpr int AVG_CHUNK = 32;            // members of a class per partial sum
constexpr int ALIGN_C_MAX = 1024;        // channels

static inline int align_tiles(int n) { return (n * n + ALIGN_TILE - 1) / ALIGN_TILE; }
static inline long avg_slots(int N, int K) { return (long)N / AVG_CHUNK + K; }

// grid = N * C * tiles (tile fastest).  out[N][C][n][n]
__global__ __launch_bounds__(ALIGN_TILE) void align_stack_kernel(const float* __restrict__ Y,
                                                                 const float* __restrict__ theta,
                                                                 const float* __restrict__ dx, float* __restrict__ out,
                                                                 int C, int n, int tiles, float t_scale) {
    __shared__ AlignPose pose;
    const int tile = blockIdx.x % tiles;
    const long plane = blockIdx.x / tiles;                    // image * C + channel
    const int img_i = (int)(plane / C);
    if (threadIdx.x == 0) {
        const float th = theta[img_i];
        pose.c = cosf(th);
        pose.s = sinf(th);
        pose.tx = t_scale * dx[2 * (long)img_i];
        pose.ty = t_scale * dx[2 * (long)img_i + 1];
    }
    __syncthreads();
    const int p = tile * ALIGN_TILE + threadIdx.x;
    if (p >= n * n) return;
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const size_t off = (size_t)plane * n * n;
    out[off + p] = align_sample(Y + off, n, p / n, p % n, step, half, pose, true);
}

// ONE workgroup.  clean[k] = min(max(0, seg[0], ..., seg[k]), N)
__global__ __launch_bounds__(ALIGN_TILE) void avg_seg_kernel(const int* __restrict__ seg, int* __restrict__ clean, int K,
                                                             int N) {
    __shared__ int part[ALIGN_TILE];
    const int len = K + 1;
    const int per = (len + ALIGN_TILE - 1) / ALIGN_TILE;
    const int lo = threadIdx.x * per, hi = min(lo + per, len);
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

// The prologue of a workgroup of avg_accum_kernel and halves_accum_kernel (grid = slots * C * tiles, tile fastest, then
// channel): which pixel tile, channel and slot `block` is, the class that owns the slot and the chunk's members; the members'
// image indices (-1 = skipped or behind the chunk's end) and poses go to LDS.  load() returns false for a slot that has no
// chunk, BEFORE any barrier: both such returns depend on `block` and `clean` alone, so they are uniform over the workgroup
// and the caller returns at once.  Otherwise it ends with the __syncthreads() behind which pose and member may be read.
struct AvgChunk {
    int tile, ch, slot, members;
    __device__ __forceinline__ bool load(unsigned block, const int* clean, const int* order, const float* theta,
                                         const float* dx, int N, int C, int K, int tiles, float t_scale, AlignPose* pose,
                                         int* member) {
        tile = block % tiles;
        const long rest = block / tiles;
        ch = (int)(rest % C);
        slot = (int)(rest / C);
        ChunkSpan span;
        if (!chunk_of_slot(clean, K, slot, AVG_CHUNK, span)) return false;   // a slot that no chunk owns
        const int first = span.first;
        members = span.members;
        if (threadIdx.x < AVG_CHUNK) {
            int id = -1;
            AlignPose q = {0.f, 0.f, 0.f, 0.f};
            if ((int)threadIdx.x < members) {
                id = order[first + threadIdx.x];
                if (id < 0 || id >= N) id = -1;
            }
            if (id >= 0) {
                const float th = theta[id];
                q.c = cosf(th);
                q.s = sinf(th);
                q.tx = t_scale * dx[2 * (long)id];
                q.ty = t_scale * dx[2 * (long)id + 1];
            }
            pose[threadIdx.x] = q;
            member[threadIdx.x] = id;
        }
        __syncthreads();
        return true;
    }
};

// grid = slots * C * tiles (tile fastest, then channel).  part[slots][C][n][n], cnt[slots] (written by tile 0 of channel 0)
__global__ __launch_bounds__(ALIGN_TILE) void avg_accum_kernel(const float* __restrict__ Y,
                                                               const float* __restrict__ theta,
                                                               const float* __restrict__ dx,
                                                               const int* __restrict__ order,
                                                               const int* __restrict__ clean, float* __restrict__ part,
                                                               int* __restrict__ cnt, int N, int C, int n, int K, int tiles,
                                                               float t_scale) {
    __shared__ AlignPose pose[AVG_CHUNK];
    __shared__ int member[AVG_CHUNK];
    AvgChunk w;
    if (!w.load(blockIdx.x, clean, order, theta, dx, N, C, K, tiles, t_scale, pose, member)) return;
    const int tile = w.tile, ch = w.ch, slot = w.slot, members = w.members;
    if (tile == 0 && ch == 0 && threadIdx.x == 0) {
        int v = 0;
        for (int m = 0; m < members; ++m) v += member[m] >= 0;
        cnt[slot] = v;
    }
    const int p = tile * ALIGN_TILE + threadIdx.x;
    if (p >= n * n) return;
    const int i = p / n, j = p % n;
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const size_t nn = (size_t)n * n;
    float acc = 0.f;
#pragma unroll 4
    for (int m = 0; m < members; ++m) {
        const int id = member[m];
        const bool on = id >= 0;
        const float* img = Y + ((size_t)(on ? id : 0) * C + ch) * nn;
        acc += align_sample(img, n, i, j, step, half, pose[m], on);
    }
    part[((size_t)slot * C + ch) * nn + p] = acc;
}

// grid = K * C * tiles (tile fastest).  avg[K][C][n][n]
__global__ __launch_bounds__(ALIGN_TILE) void avg_reduce_kernel(const float* __restrict__ part,
                                                                const int* __restrict__ cnt,
                                                                const int* __restrict__ clean, float* __restrict__ avg,
                                                                int C, int n, int tiles) {
    const int tile = blockIdx.x % tiles;
    const long plane = blockIdx.x / tiles;                    // class * C + channel
    const int k = (int)(plane / C), ch = (int)(plane % C);
    const int p = tile * ALIGN_TILE + threadIdx.x;
    if (p >= n * n) return;
    const int sk = clean[k], ek = clean[k + 1];
    const int chunks = (ek - sk + AVG_CHUNK - 1) / AVG_CHUNK;
    const int slot0 = sk / AVG_CHUNK + k;
    const size_t nn = (size_t)n * n;
    float sum = 0.f;
    int members = 0;
    for (int c = 0; c < chunks; ++c) {
        sum += part[((size_t)(slot0 + c) * C + ch) * nn + p];
        members += cnt[slot0 + c];
    }
    avg[(size_t)plane * nn + p] = members > 0 ? sum / (float)members : 0.f;
}

}  // namespace tvae_cluster
