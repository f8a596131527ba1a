// Particle preprocessing (include/tvae_cluster.h, last section): the batched sandwich product out = scale (Ar X Br - Ai X Bi)
// that a Fourier crop to a fixed size is, and the background-ring normalisation.
//
// image_resample_kernel.  One 256-thread workgroup (four waves) owns a 64 x TN tile of ONE image's output, TN = 64 NJ, and
// walks the window in chunks of 64 columns:
//   stage 1   U = Ar[64 rows][M] X[M][chunk]  (and V = Ai ...), the reduction over the window's rows in steps of 16: the Ar / Ai
//             tiles [16][64] and the X tile [16][64] go global -> registers -> LDS (k-major, 68-float rows: the fragment reads of
//             32 consecutive x at a fixed k are conflict-free), the next step's loads are in flight under this step's MFMAs;
//             IMAG: wave w holds the (w & 1) row half of U (w < 2) or V (w >= 2), both column halves; without the second term
//             wave w holds row half (w & 1), column half (w >> 1) of U;
//   hand-over U, V -> LDS row-major [64][65] (the accumulator's lanes run along the chunk column: conflict-free writes, and the
//             A-fragment reads of stage 2 walk rows at stride 65: conflict-free as well);
//   stage 2   acc += U Br[chunk][TN] - V Bi[chunk][TN] in steps of 16 chunk columns, the Br / Bi tiles staged like stage 1's;
//             wave (w >> 1, w & 1) owns 32 rows x TN / 2 columns of the tile in registers for the whole walk.
// v_mfma_f32_32x32x2_f32 throughout (an exact fp32 FMA chain per output, ascending k; the fragment layout: cluster_common.hpp).
// Every element outside the window, the tables or the output is a PREDICATED zero: nothing outside a tensor or outside the
// window is ever loaded.  LDS: 50 KB whatever the shape.  No atomics; an output depends on its image and the tables only.
//
// image_norm_*_kernel.  An image is cut into groups of IMG_NORM_GROUP pixels; three launches over (group, image): the masked
// count and sum of a group; the masked sum of (x - mu)^2 of a group, mu from the partials of ALL groups of the image in
// ascending order; the pixels (x - mu) / sigma.  fp64 throughout, per-thread sums in ascending pixel order, then a fixed tree.
#pragma once
#include <hip/hip_runtime.h>

#include "cluster_common.hpp"

namespace tvae_cluster {

constexpr int IMG_THREADS = 256;
constexpr int IMG_TM = 64;          // output rows of a workgroup
constexpr int IMG_CK = 64;          // window columns of a chunk
constexpr int IMG_BK = 16;          // reduction step of both stages
constexpr int IMG_LD = 68;          // k-major staging tile [16][64 + 4]
constexpr int IMG_UV_LD = 65;       // U, V [64][64 + 1]
constexpr int IMG_NORM_GROUP = 4096;

static inline int img_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int img_nj(int n) { return n > 64 ? 2 : 1; }

// One [16][64] tile, element (k, x), of a row-major matrix.  XFAST: element at p[k * ld + x] (x contiguous: the window, Br, Bi);
// thread -> x = tid & 63, k = (tid >> 6) + 4 j.  Otherwise element at p[x * ld + k] (k contiguous: Ar, Ai); thread -> k = tid & 15,
// x = (tid >> 4) + 16 j.  k < klim and x < xlim are in range; anything else is zero and is not loaded.
template <bool XFAST>
struct ImgTile {
    float r[4];
    __device__ __forceinline__ void fetch(const float* __restrict__ p, long ld, int k0, int klim, int x0, int xlim, int tid) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + (XFAST ? (tid >> 6) + 4 * j : (tid & 15));
            const int x = x0 + (XFAST ? (tid & 63) : (tid >> 4) + 16 * j);
            const bool ok = k < klim && x < xlim;
            r[j] = 0.f;
            if (ok) r[j] = XFAST ? p[(long)k * ld + x] : p[(long)x * ld + k];
        }
    }
    __device__ __forceinline__ void commit(float* S, int tid) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = XFAST ? (tid >> 6) + 4 * j : (tid & 15);
            const int x = XFAST ? (tid & 63) : (tid >> 4) + 16 * j;
            S[k * IMG_LD + x] = r[j];
        }
    }
};

template <int NJ, bool IMAG>
static __global__ __launch_bounds__(IMG_THREADS, 2)
void image_resample_kernel(const float* __restrict__ X, const float* __restrict__ Ar, const float* __restrict__ Ai,
                           const float* __restrict__ Br, const float* __restrict__ Bi, float* __restrict__ out, int H, int W,
                           int r0, int c0, int M, int N, int m, int n, float scale, int tiles_m, int tiles_n) {
    constexpr int TILE = IMG_BK * IMG_LD;                     // floats of one staged [16][64] tile
    constexpr int STAGE = (2 * NJ * TILE > 3 * TILE) ? 2 * NJ * TILE : 3 * TILE;
    __shared__ float lds[STAGE + 2 * IMG_TM * IMG_UV_LD];
    float* const uv = lds + STAGE;                            // U then V, [64][65] each

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const unsigned tiles = (unsigned)(tiles_m * tiles_n);
    const unsigned img = blockIdx.x / tiles, t = blockIdx.x - img * tiles;
    const int i0 = (int)(t / tiles_n) * IMG_TM, j0 = (int)(t % tiles_n) * (64 * NJ);
    const float* __restrict__ xw = X + ((long)img * H + r0) * W + c0;        // the window's (0, 0)

    const int wm = wave >> 1, wn = wave & 1;                  // stage 2: rows wm 32 .., columns wn 32 NJ ..
    f32x16 acc[NJ];
#pragma unroll
    for (int q = 0; q < NJ; ++q) zero(acc[q]);

    // stage 1 roles
    const int s1_rows = (wave & 1) * 32;
    const int s1_part = IMAG ? (wave >> 1) : 0;               // 0: U from Ar, 1: V from Ai
    constexpr int NC1 = IMAG ? 2 : 1;                         // column halves of the chunk a wave computes
    const int s1_col0 = IMAG ? 0 : (wave >> 1) * 32;

    ImgTile<false> ta, tb;
    ImgTile<true> tx, tq[2 * NJ];

    for (int cc = 0; cc < N; cc += IMG_CK) {
        // ---- stage 1 ------------------------------------------------------------------------------------------------
        f32x16 u[NC1];
#pragma unroll
        for (int q = 0; q < NC1; ++q) zero(u[q]);
        const int nk = (M + IMG_BK - 1) / IMG_BK;
        ta.fetch(Ar, M, 0, M, i0, m, tid);
        if (IMAG) tb.fetch(Ai, M, 0, M, i0, m, tid);
        tx.fetch(xw, W, 0, M, cc, N, tid);
        for (int ks = 0; ks < nk; ++ks) {
            __syncthreads();                                  // the previous readers of the staging tiles are done
            ta.commit(lds, tid);
            if (IMAG) tb.commit(lds + TILE, tid);
            tx.commit(lds + 2 * TILE, tid);
            __syncthreads();
            if (ks + 1 < nk) {
                const int k0 = (ks + 1) * IMG_BK;
                ta.fetch(Ar, M, k0, M, i0, m, tid);
                if (IMAG) tb.fetch(Ai, M, k0, M, i0, m, tid);
                tx.fetch(xw, W, k0, M, cc, N, tid);
            }
            const float* as = lds + s1_part * TILE + s1_rows + l31;
            const float* xs = lds + 2 * TILE + s1_col0 + l31;
#pragma unroll
            for (int s = 0; s < IMG_BK / 2; ++s) {
                const int kk = 2 * s + khalf;
                const float a = as[kk * IMG_LD];
#pragma unroll
                for (int q = 0; q < NC1; ++q)
                    u[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xs[kk * IMG_LD + 32 * q], u[q], 0, 0, 0);
            }
        }
        // ---- hand-over: U (and V) of this chunk, row-major ------------------------------------------------------------
        // (uv's last readers, stage 2 of the previous chunk, are behind the barriers of the loop above: nk >= 1)
#pragma unroll
        for (int q = 0; q < NC1; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma_row(r, khalf, s1_rows);
                uv[s1_part * (IMG_TM * IMG_UV_LD) + row * IMG_UV_LD + s1_col0 + 32 * q + l31] = u[q][r];
            }
        // ---- stage 2 ------------------------------------------------------------------------------------------------
        const int ck = min(IMG_CK, N - cc);                   // chunk columns in range; the rest of U, V is zero
        const int nk2 = (ck + IMG_BK - 1) / IMG_BK;
        auto fetch2 = [&](int k0) {
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                tq[q].fetch(Br + (long)cc * n, n, k0, ck, j0 + 64 * q, n, tid);
                if (IMAG) tq[NJ + q].fetch(Bi + (long)cc * n, n, k0, ck, j0 + 64 * q, n, tid);
            }
        };
        fetch2(0);
        for (int ks = 0; ks < nk2; ++ks) {
            __syncthreads();                                  // stage 1's (or the previous step's) readers are done; uv is written
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                tq[q].commit(lds + q * TILE, tid);
                if (IMAG) tq[NJ + q].commit(lds + (NJ + q) * TILE, tid);
            }
            __syncthreads();
            if (ks + 1 < nk2) fetch2((ks + 1) * IMG_BK);
            const float* us = uv + (wm * 32 + l31) * IMG_UV_LD + ks * IMG_BK;
            const float* bs = lds + wn * 32 + l31;            // column wn 32 + 64 q + l31 of the tile: tile q, offset wn 32
#pragma unroll
            for (int s = 0; s < IMG_BK / 2; ++s) {
                const int kk = 2 * s + khalf;
                const float a = us[kk];
#pragma unroll
                for (int q = 0; q < NJ; ++q)
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bs[q * TILE + kk * IMG_LD], acc[q], 0, 0, 0);
            }
            if (IMAG) {
#pragma unroll
                for (int s = 0; s < IMG_BK / 2; ++s) {
                    const int kk = 2 * s + khalf;
                    const float a = -us[IMG_TM * IMG_UV_LD + kk];
#pragma unroll
                    for (int q = 0; q < NJ; ++q)
                        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bs[(NJ + q) * TILE + kk * IMG_LD], acc[q], 0, 0, 0);
                }
            }
        }
    }

    float* __restrict__ o = out + (long)img * m * n;
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        const int j = j0 + 64 * q + wn * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = mfma_row(r, khalf, i0 + wm * 32);
            if (i < m && j < n) o[(long)i * n + j] = scale * acc[q][r];
        }
    }
}

// ---- normalisation -------------------------------------------------------------------------------------------------------
// fixed tree over the 256 threads' fp64 values; the result is valid in every thread
__device__ __forceinline__ double img_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // an earlier result has been read
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = IMG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// the mask of pixel p = i m + j of an n x m image: (n / 2 - i)^2 + (m / 2 - j)^2 >= r2, exact in fp64
__device__ __forceinline__ bool img_in_ring(int p, int n, int m, double r2) {
    const int i = p / m, j = p - i * m;
    const double dy = 0.5 * n - i, dx = 0.5 * m - j;
    return dy * dy + dx * dx >= r2;
}

// part[image][group][3] = (masked count, masked sum, masked sum of squared deviations); this launch writes the first two
static __global__ __launch_bounds__(IMG_THREADS)
void image_norm_sum_kernel(const float* __restrict__ X, double* __restrict__ part, int n, int m, int G, double r2) {
    __shared__ double red[IMG_THREADS];
    const unsigned b = blockIdx.x / G, g = blockIdx.x - b * G;
    const int P = n * m, pend = min(P, (int)(g + 1) * IMG_NORM_GROUP);
    const float* __restrict__ x = X + (long)b * P;
    double cnt = 0.0, s = 0.0;
    for (int p = (int)g * IMG_NORM_GROUP + threadIdx.x; p < pend; p += IMG_THREADS)
        if (img_in_ring(p, n, m, r2)) { cnt += 1.0; s += (double)x[p]; }
    cnt = img_block_sum(cnt, red);
    s = img_block_sum(s, red);
    if (threadIdx.x == 0) {
        part[(long)blockIdx.x * 3 + 0] = cnt;
        part[(long)blockIdx.x * 3 + 1] = s;
    }
}

// (count, mean) of image b from the partials of all its groups, ascending
__device__ __forceinline__ void img_mean(const double* __restrict__ part, unsigned b, int G, double& cnt, double& mu) {
    double c = 0.0, s = 0.0;
    for (int q = 0; q < G; ++q) {
        c += part[((long)b * G + q) * 3 + 0];
        s += part[((long)b * G + q) * 3 + 1];
    }
    cnt = c;
    mu = s / c;
}

static __global__ __launch_bounds__(IMG_THREADS)
void image_norm_dev_kernel(const float* __restrict__ X, double* __restrict__ part, int n, int m, int G, double r2) {
    __shared__ double red[IMG_THREADS];
    const unsigned b = blockIdx.x / G, g = blockIdx.x - b * G;
    const int P = n * m, pend = min(P, (int)(g + 1) * IMG_NORM_GROUP);
    const float* __restrict__ x = X + (long)b * P;
    double cnt, mu;
    img_mean(part, b, G, cnt, mu);
    double q = 0.0;
    for (int p = (int)g * IMG_NORM_GROUP + threadIdx.x; p < pend; p += IMG_THREADS)
        if (img_in_ring(p, n, m, r2)) { const double d = (double)x[p] - mu; q += d * d; }
    q = img_block_sum(q, red);
    if (threadIdx.x == 0) part[(long)blockIdx.x * 3 + 2] = q;
}

// out may be X: a thread reads the pixel it writes and nothing else of the image
static __global__ __launch_bounds__(IMG_THREADS)
void image_norm_apply_kernel(const float* X, float* out, double* __restrict__ stats, const double* __restrict__ part, int n,
                             int m, int G) {
    const unsigned b = blockIdx.x / G, g = blockIdx.x - b * G;
    const int P = n * m, pend = min(P, (int)(g + 1) * IMG_NORM_GROUP);
    double cnt, mu, q = 0.0;
    img_mean(part, b, G, cnt, mu);
    for (int k = 0; k < G; ++k) q += part[((long)b * G + k) * 3 + 2];
    const double sigma = sqrt(q / cnt);
    const float* x = X + (long)b * P;
    float* o = out + (long)b * P;
    for (int p = (int)g * IMG_NORM_GROUP + threadIdx.x; p < pend; p += IMG_THREADS) o[p] = (float)(((double)x[p] - mu) / sigma);
    if (g == 0 && threadIdx.x == 0) {
        stats[2L * b + 0] = mu;
        stats[2L * b + 1] = sigma;
    }
}

}  // namespace tvae_cluster
