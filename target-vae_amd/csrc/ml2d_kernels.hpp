// Maximum-likelihood 2-D class averages (libtvae_cluster.so): the E-step over the tables of tvae_pose_classify and the
// M-step, a weighted aligned average over a list of (image, pose, weight) entries.  include/tvae_cluster.h states both
// definitions.  Included by abi_ml2d.hip only.
//
// posterior_kernel      a workgroup = one image, 256 threads.  l_j = logprior - r_j / (2 sigma^2) in fp64 for the J = M NA NS^2
//                       candidates; J <= POST_CACHE keeps them in LDS, a larger J forms them again where they are needed, by
//                       the same function under contract(off): the same bits.  Three passes: the maximum (and every thread's
//                       own best candidate); per slot the sums of e = exp(l - L) and e r, thread t adding the slot's candidates
//                       t, t + 256, ... in one chain and a binary tree above the 256 chains; the selection, P times the best of
//                       the 256 threads' best, after which only the thread that owned the winner looks for its next one.
// wavg_seg_kernel       ONE workgroup: clean[k] = min(max(0, seg[0], ..., seg[k]), E), the rule of avg_seg_kernel.
// wavg_accum_kernel     a workgroup = 256 pixels x one channel x one chunk of WAVG_CHUNK entries of a class, as
//                       avg_accum_kernel: the entries' poses and weights in LDS, acc = fma(w, a, acc) in ascending entry; the
//                       workgroup of tile 0 and channel 0 adds the chunk's live weights in fp64 and counts them.
// wavg_reduce_kernel    a thread = a pixel of avg[k][ch]: the class's chunks in ascending order in fp64, divided by the weight.
// Chunks and slots by chunk_of_slot of cluster_common.hpp with WAVG_CHUNK entries per chunk and E for N: chunk c of class k owns
// the slot floor(s_k / WAVG_CHUNK) + k + c.  No atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include "refine_device.hpp"          // the pose of a candidate (refine_write_pose) and, through it, cluster_common.hpp

// every product and sum of this file is rounded on its own; a fused multiply-add is an fma() or fmaf()
#pragma clang fp contract(off)

namespace tvae_cluster {

constexpr int POST_TILE = 256;           // threads per workgroup
constexpr int POST_M_MAX = TVAE_CLASSIFY_MAX_CANDIDATES;
constexpr int POST_KEEP_MAX = TVAE_POSTERIOR_MAX_KEEP;
constexpr int POST_CACHE = 4096;         // candidates whose l stays in LDS (32 KB)

__device__ __forceinline__ bool post_finite(double x) { return x - x == 0.0; }

// the rank order: l descending, then j ascending; j < 0 is nobody
__device__ __forceinline__ bool post_before(double la, int ja, double lb, int jb) {
    return ja >= 0 && (jb < 0 || la > lb || (la == lb && ja < jb));
}

// what a workgroup knows of its image; scls [M] the class of a slot or -1, slp [M] its log prior (LDS)
struct PostImage {
    const float* nu;
    const float* p;
    const int* scls;
    const double* slp;
    double y, h;
    int cnd;
    __device__ __forceinline__ double r(int j) const { return ((y - 2.0 * (double)nu[j]) + (double)p[j]); }
    // l of candidate j, NaN for one that is not live
    __device__ __forceinline__ double l(int j) const {
        const int m = j / cnd;
        if (scls[m] < 0) return __builtin_nan("");
        const double v = slp[m] - r(j) * h;
        return post_finite(v) ? v : __builtin_nan("");
    }
};

// The first in rank order of the 256 (l, j) of the threads -> red[0], redj[0], to be read behind the barrier this ends with.
// Every thread of the workgroup calls it; it begins with a barrier, so red and redj may still be being read.
__device__ __forceinline__ void post_first(double* red, int* redj, double l, int j, int tid) {
    __syncthreads();
    red[tid] = l;
    redj[tid] = j;
    __syncthreads();
    for (int w = POST_TILE / 2; w > 0; w >>= 1) {
        if (tid < w && post_before(red[tid + w], redj[tid + w], red[tid], redj[tid])) {
            red[tid] = red[tid + w];
            redj[tid] = redj[tid + w];
        }
        __syncthreads();
    }
}

// grid = N.  num, pp [N][M][NA][NS][NS], yy [N], cand [N][M], logprior [K] or NULL; ent_* [N][P] (ent_dx [N][P][2]),
// resp [N][M], lse, r2, kept [N]
__global__ __launch_bounds__(POST_TILE) void posterior_kernel(
    const float* __restrict__ num, const float* __restrict__ pp, const float* __restrict__ yy, const int* __restrict__ cand,
    const double* __restrict__ logprior, const float* __restrict__ theta, const float* __restrict__ dx,
    int* __restrict__ ent_idx, int* __restrict__ ent_cls, float* __restrict__ ent_theta, float* __restrict__ ent_dx,
    float* __restrict__ ent_w, float* __restrict__ resp, double* __restrict__ lse, double* __restrict__ r2,
    float* __restrict__ kept, int n, int K, int M, int A, int S, int P, float t_scale, float dtheta, float sigma2) {
    __shared__ double lc[POST_CACHE];
    __shared__ double red[POST_TILE], red2[POST_TILE];
    __shared__ int redj[POST_TILE];
    __shared__ double slp[POST_M_MAX], es[POST_M_MAX], rs[POST_M_MAX];
    __shared__ int scls[POST_M_MAX];
    __shared__ double selw[POST_KEEP_MAX];
    __shared__ int selj[POST_KEEP_MAX];
    const int tid = threadIdx.x, img = blockIdx.x;
    const int NS = 2 * S + 1, cnd = (2 * A + 1) * NS * NS, J = M * cnd;
    const bool cached = J <= POST_CACHE;
    if (tid < M) {
        const int k = cand[(size_t)img * M + tid];
        const bool ok = k >= 0 && k < K;
        scls[tid] = ok ? k : -1;
        slp[tid] = (ok && logprior) ? logprior[k] : 0.0;
    }
    __syncthreads();
    PostImage I;
    I.nu = num + (size_t)img * J;
    I.p = pp + (size_t)img * J;
    I.scls = scls;
    I.slp = slp;
    I.y = (double)yy[img];
    I.h = 0.5 / (double)sigma2;
    I.cnd = cnd;
    const size_t ebase = (size_t)img * P;
    const float th = theta[img], d0 = dx[2 * (size_t)img], d1 = dx[2 * (size_t)img + 1];

    // ---- the maximum, and the first candidate of every thread's own share ----------------------------------------------------
    double bl = 0.0;
    int bj = -1;
    for (int j = tid; j < J; j += POST_TILE) {
        const double l = I.l(j);
        if (cached) lc[j] = l;
        if (post_finite(l) && (bj < 0 || l > bl)) {           // ascending j: a tie stays with the lower j
            bl = l;
            bj = j;
        }
    }
    post_first(red, redj, bl, bj, tid);
    if (redj[0] < 0) {                                        // no live candidate (uniform): zeros and empty entries
        if (tid < P) {
            ent_idx[ebase + tid] = -1;
            ent_cls[ebase + tid] = -1;
            ent_w[ebase + tid] = 0.f;
            refine_write_pose(ent_theta + ebase, ent_dx + 2 * ebase, tid, th, d0, d1, 0, 0, 0, n, t_scale, dtheta);
        }
        if (tid < M) resp[(size_t)img * M + tid] = 0.f;
        if (tid == 0) {
            lse[img] = 0.0;
            r2[img] = 0.0;
            kept[img] = 0.f;
        }
        return;
    }
    const double L = red[0];

    // ---- per slot: E_m = sum e and R_m = sum e r -----------------------------------------------------------------------------
    for (int m = 0; m < M; ++m) {
        double a = 0.0, b = 0.0;
        if (scls[m] >= 0) {                                   // (uniform)
            for (int c = tid; c < cnd; c += POST_TILE) {
                const int j = m * cnd + c;
                const double l = cached ? lc[j] : I.l(j);
                if (post_finite(l)) {
                    const double e = exp(l - L);
                    a = a + e;
                    b = b + e * I.r(j);
                }
            }
        }
        __syncthreads();                                      // red[0] and red2[0] of the slot before have been taken
        red[tid] = a;
        red2[tid] = b;
        __syncthreads();
        for (int w = POST_TILE / 2; w > 0; w >>= 1) {
            if (tid < w) {
                red[tid] += red[tid + w];
                red2[tid] += red2[tid + w];
            }
            __syncthreads();
        }
        if (tid == 0) {
            es[m] = red[0];
            rs[m] = red2[0];
        }
    }
    __syncthreads();
    double Z = 0.0, R = 0.0;                                  // ascending slot, every thread for itself
    for (int m = 0; m < M; ++m) {
        Z = Z + es[m];
        R = R + rs[m];
    }
    if (tid < M) resp[(size_t)img * M + tid] = (float)(es[tid] / Z);
    if (tid == 0) {
        lse[img] = L + log(Z);
        r2[img] = R / Z;
    }

    // ---- the first P in rank order ---------------------------------------------------------------------------------------------
    int got = 0;
    for (; got < P; ++got) {
        post_first(red, redj, bl, bj, tid);
        const double wl = red[0];
        const int wj = redj[0];
        if (wj < 0) break;                                    // (uniform) fewer than P live candidates
        if (tid == 0) {
            selj[got] = wj;
            selw[got] = exp(wl - L) / Z;
        }
        if (wj % POST_TILE == tid) {                          // the owner: its first candidate behind the winner
            bl = 0.0;
            bj = -1;
            for (int j = tid; j < J; j += POST_TILE) {
                const double l = cached ? lc[j] : I.l(j);
                if (post_finite(l) && (l < wl || (l == wl && j > wj)) && (bj < 0 || l > bl)) {
                    bl = l;
                    bj = j;
                }
            }
        }
    }
    __syncthreads();
    double W = 0.0;                                           // rank order, every thread for itself
    for (int q = 0; q < got; ++q) W = W + selw[q];
    if (tid == 0) kept[img] = (float)W;
    if (tid < P) {
        int a = 0, sy = 0, sx = 0, j = -1, k = -1;
        float w = 0.f;
        if (tid < got) {
            j = selj[tid];
            const int m = j / cnd, c = j - m * cnd;
            a = c / (NS * NS) - A;
            sy = (c / NS) % NS - S;
            sx = c % NS - S;
            k = scls[m];
            w = (float)(selw[tid] / W);
        }
        ent_idx[ebase + tid] = j;
        ent_cls[ebase + tid] = k;
        ent_w[ebase + tid] = w;
        refine_write_pose(ent_theta + ebase, ent_dx + 2 * ebase, tid, th, d0, d1, a, sy, sx, n, t_scale, dtheta);
    }
}

// ---- the weighted average ---------------------------------------------------------------------------------------------------------
constexpr int WAVG_TILE = 256;           // pixels per workgroup = threads per workgroup
constexpr int WAVG_CHUNK = 128;          // entries of a class per partial sum (E is several times N: four times AVG_CHUNK)
constexpr int WAVG_C_MAX = 1024;         // channels, as ALIGN_C_MAX
constexpr long WAVG_E_MAX = 1L << 30;

static inline int wavg_tiles(int n) { return (n * n + WAVG_TILE - 1) / WAVG_TILE; }
static inline long wavg_slots(long E, int K) { return E / WAVG_CHUNK + K; }

// ONE workgroup.  clean[k] = min(max(0, seg[0], ..., seg[k]), E)
__global__ __launch_bounds__(WAVG_TILE) void wavg_seg_kernel(const int* __restrict__ seg, int* __restrict__ clean, int K,
                                                             int E) {
    __shared__ int part[WAVG_TILE];
    const int len = K + 1;
    const int per = (len + WAVG_TILE - 1) / WAVG_TILE;
    const int lo = min((int)threadIdx.x * per, len), hi = min(lo + per, len);
    int m = 0;
    for (int k = lo; k < hi; ++k) m = max(m, seg[k]);
    part[threadIdx.x] = m;
    __syncthreads();
    int run = 0;                                              // maximum of everything in front of this thread's share
    for (int t = 0; t < (int)threadIdx.x; ++t) run = max(run, part[t]);
    for (int k = lo; k < hi; ++k) {
        run = max(run, seg[k]);
        clean[k] = min(run, E);
    }
}

// grid = slots * C * tiles (tile fastest, then channel).  part[slots][C][n][n]; wpart[slots] and cnt[slots] are written by
// tile 0 of channel 0
__global__ __launch_bounds__(WAVG_TILE) void wavg_accum_kernel(
    const float* __restrict__ Y, const int* __restrict__ img, const float* __restrict__ theta_e,
    const float* __restrict__ dx_e, const float* __restrict__ w, const int* __restrict__ clean, float* __restrict__ part,
    double* __restrict__ wpart, int* __restrict__ cnt, int N, int C, int n, int K, int tiles, float t_scale) {
    __shared__ AlignPose pose[WAVG_CHUNK];
    __shared__ int member[WAVG_CHUNK];
    __shared__ float wt[WAVG_CHUNK];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles;
    const long rest = blockIdx.x / tiles;
    const int ch = (int)(rest % C), slot = (int)(rest / C);
    // The return depends on blockIdx and `clean` alone: uniform over the workgroup, in front of every barrier.
    ChunkSpan span;
    if (!chunk_of_slot(clean, K, slot, WAVG_CHUNK, span)) return;        // a slot that no chunk owns
    const int first = span.first, members = span.members;
    if (tid < WAVG_CHUNK) {
        int id = -1;
        float wv = 0.f;
        AlignPose q = {0.f, 0.f, 0.f, 0.f};
        if (tid < members) {
            const int e = first + tid;
            id = img[e];
            wv = w[e];
            if (id < 0 || id >= N || !(wv - wv == 0.f) || !(wv > 0.f)) id = -1;       // dead: nothing of it counts
            if (id >= 0) {
                const float th = theta_e[e];
                q.c = cosf(th);
                q.s = sinf(th);
                q.tx = t_scale * dx_e[2 * (long)e];
                q.ty = t_scale * dx_e[2 * (long)e + 1];
            } else {
                wv = 0.f;
            }
        }
        pose[tid] = q;
        member[tid] = id;
        wt[tid] = wv;
    }
    __syncthreads();
    if (tile == 0 && ch == 0 && tid == 0) {
        int v = 0;
        double s = 0.0;
        for (int m = 0; m < members; ++m) {
            if (member[m] >= 0) {
                v += 1;
                s = s + (double)wt[m];
            }
        }
        cnt[slot] = v;
        wpart[slot] = s;
    }
    const int p = tile * WAVG_TILE + tid;
    if (p >= n * n) return;
    const int i = p / n, j = p % n;
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const size_t nn = (size_t)n * n;
    float acc = 0.f;
#pragma unroll 4
    for (int m = 0; m < members; ++m) {
        const int id = member[m];
        const bool on = id >= 0;
        const float* src = Y + ((size_t)(on ? id : 0) * C + ch) * nn;
        acc = fmaf(wt[m], align_sample(src, n, i, j, step, half, pose[m], on), acc);
    }
    part[((size_t)slot * C + ch) * nn + p] = acc;
}

// grid = K * C * tiles (tile fastest).  avg[K][C][n][n], wsum[K], counts[K]
__global__ __launch_bounds__(WAVG_TILE) void wavg_reduce_kernel(const float* __restrict__ part,
                                                                const double* __restrict__ wpart,
                                                                const int* __restrict__ cnt, const int* __restrict__ clean,
                                                                float* __restrict__ avg, double* __restrict__ wsum,
                                                                int* __restrict__ counts, int C, int n, int tiles) {
    const int tile = blockIdx.x % tiles;
    const long plane = blockIdx.x / tiles;                    // class * C + channel
    const int k = (int)(plane / C), ch = (int)(plane % C);
    const int sk = clean[k], ek = clean[k + 1];
    const int chunks = (ek - sk + WAVG_CHUNK - 1) / WAVG_CHUNK;
    const int slot0 = sk / WAVG_CHUNK + k;
    if (tile == 0 && ch == 0 && threadIdx.x == 0) {
        double W = 0.0;
        int members = 0;
        for (int c = 0; c < chunks; ++c) {
            W = W + wpart[slot0 + c];
            members += cnt[slot0 + c];
        }
        wsum[k] = W;
        counts[k] = members;
    }
    const int p = tile * WAVG_TILE + threadIdx.x;
    if (p >= n * n) return;
    const size_t nn = (size_t)n * n;
    double sum = 0.0, W = 0.0;
    for (int c = 0; c < chunks; ++c) {
        sum = sum + (double)part[((size_t)(slot0 + c) * C + ch) * nn + p];
        W = W + wpart[slot0 + c];
    }
    avg[(size_t)plane * nn + p] = W > 0.0 ? (float)(sum / W) : 0.f;
}

}  // namespace tvae_cluster
