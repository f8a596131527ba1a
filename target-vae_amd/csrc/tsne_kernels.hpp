// Exact t-SNE of the latents (libtvae_cluster.so): brute-force k nearest neighbours for the sparse input similarities and
// the all-pairs repulsion of the 2-D embedding, both without an N x N matrix.
//
// knn_kernel            ONE wave per workgroup, a lane = a row (its features in registers for d <= DREG).  Column tiles
//                       stream through LDS feature-major exactly as in ward_nn_kernel; the running top-K of every row is a
//                       sorted list in LDS, [K][rows] (lane l only touches word l of a list row: no bank conflict inside
//                       a 32-lane group).  A candidate enters iff its distance is STRICTLY below the current K-th one and
//                       is shifted in behind every entry of equal distance: columns arrive in ascending j, so the list is
//                       sorted by (d2, index) and ties go to the lowest index.  j == i is excluded by index.
// tsne_repulsion_kernel a lane = a row i, a workgroup = 256 rows x one range of column tiles; the y_j of a tile are
//                       wave-uniform and come from LDS as 16-byte broadcast reads.  Per pair q = 1 / (1 + |y_i - y_j|^2)
//                       (v_rcp_f32), rep += q^2 (y_i - y_j), z += q; only the tiles that overlap the workgroup's own rows
//                       (or the end of the points) pay for the index test.  Partials [S][3][N] in fp32.
// tsne_rows_kernel      the S ranges of a row in ascending order (rep in fp32, the row's z in fp64), then the 256 rows of
//                       the workgroup in an fp64 LDS tree -> one fp64 per workgroup.
// tsne_sum_kernel       ONE workgroup adds such per-workgroup fp64 partials: a thread walks its strided share in ascending
//                       order, then the same tree.  Z, the KL divergence and every other cross-row sum go through it.
// tsne_step_kernel      a lane = a row: attraction over the row's CSR entries, gradient, sklearn's gain / momentum rule,
//                       new embedding into a SECOND buffer; |grad|^2 per workgroup in fp64.
// tsne_kl_kernel        a lane = a row: sum p ln(max(p, eps) / max(q / Z, eps)) over the row's entries in fp64.
// No float atomics anywhere; every split depends on the sizes only.
#pragma once
#include <hip/hip_runtime.h>

namespace tvae_cluster {

constexpr int KNN_WAVE = 64;             // threads per workgroup of knn_kernel = one wave
constexpr int KNN_LIST_WORDS = 12288;    // LDS words of the top-K lists (48 KB): rows * K * 2 <= this
constexpr int KNN_TILE_FLOATS = 4096;    // LDS budget of a column tile (16 KB)
constexpr int KNN_KC_MAX = 256;
constexpr int KNN_K_MAX = 256;
constexpr int TSNE_TILE = 256;           // rows per workgroup = threads per workgroup
constexpr int TSNE_KC = 512;             // columns per LDS tile of the repulsion
constexpr int TSNE_WGS = 2048;           // workgroups a repulsion launch aims at
constexpr int TSNE_N_MAX = 1 << 24;

// rows a wave keeps lists for: 64 up to K = 96, then 32, then 16 (K <= 256)
static inline int knn_rows(int K) { return K <= 96 ? 64 : (K <= 192 ? 32 : 16); }
static inline int knn_kc(int d) {
    const int kc = (KNN_TILE_FLOATS / d) & ~3;
    return kc < KNN_KC_MAX ? kc : KNN_KC_MAX;
}

struct TsnePlan {
    int RT, nct, S, tps;                 // row tiles, column tiles, column ranges, tiles per range
};

static inline TsnePlan tsne_plan(int N) {
    TsnePlan p;
    p.RT = (N + TSNE_TILE - 1) / TSNE_TILE;
    p.nct = (N + TSNE_KC - 1) / TSNE_KC;
    int want = TSNE_WGS / p.RT;
    if (want < 1) want = 1;
    const int S = want < p.nct ? want : p.nct;
    p.tps = (p.nct + S - 1) / S;
    p.S = (p.nct + p.tps - 1) / p.tps;
    return p;
}

// grid = ceil(N / rows).  idx / d2 [N][K].
template <int DREG>
__global__ __launch_bounds__(KNN_WAVE) void knn_kernel(const float* __restrict__ Xt, long ldx, int* __restrict__ idx,
                                                       float* __restrict__ d2o, int N, int d, int K, int rows, int KC,
                                                       int vec) {
    extern __shared__ __attribute__((aligned(16))) float4 knn_s4[];
    float* Cs = reinterpret_cast<float*>(knn_s4);               // [d][KC]
    float* Ld = Cs + d * KC;                                    // [K][rows]
    int* Li = reinterpret_cast<int*>(Ld + K * rows);            // [K][rows]
    const int tid = threadIdx.x;
    const int i = blockIdx.x * rows + tid;
    const bool valid = tid < rows && i < N;
    const int ic = (i < N) ? i : N - 1;
    float xr[DREG > 0 ? DREG : 1];
    if (DREG > 0) {
#pragma unroll
        for (int f = 0; f < DREG; ++f) xr[f] = (f < d) ? Xt[(long)f * ldx + ic] : 0.f;
    }
    if (tid < rows) {
        for (int p = 0; p < K; ++p) {
            Ld[p * rows + tid] = __builtin_inff();
            Li[p * rows + tid] = -1;
        }
    }
    float kth = __builtin_inff();                               // Ld[(K - 1) * rows + tid]
    for (int c0 = 0; c0 < N; c0 += KC) {
        const int kc = (N - c0 < KC) ? N - c0 : KC;
        __syncthreads();
        if (vec) {                                              // c0 % 4 == 0, ldx % 4 == 0: a quad never leaves its row
            const int K4 = KC >> 2;
            for (int q = tid; q < d * K4; q += KNN_WAVE) {
                const int f = q / K4, c4 = (q - f * K4) << 2;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c4 < kc) v = *reinterpret_cast<const float4*>(Xt + (long)f * ldx + c0 + c4);
                *reinterpret_cast<float4*>(&Cs[f * KC + c4]) = v;
            }
        } else {
            for (int q = tid; q < d * KC; q += KNN_WAVE) {
                const int f = q / KC, cc = q - f * KC;
                Cs[f * KC + cc] = (cc < kc) ? Xt[(long)f * ldx + c0 + cc] : 0.f;
            }
        }
        __syncthreads();
        for (int cc = 0; cc < kc; cc += 4) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (DREG > 0) {
#pragma unroll
                for (int f = 0; f < DREG; ++f) {
                    if (f < d) {
                        const float4 cv = *reinterpret_cast<const float4*>(&Cs[f * KC + cc]);
                        const float e0 = xr[f] - cv.x, e1 = xr[f] - cv.y, e2 = xr[f] - cv.z, e3 = xr[f] - cv.w;
                        a[0] = __builtin_fmaf(e0, e0, a[0]);
                        a[1] = __builtin_fmaf(e1, e1, a[1]);
                        a[2] = __builtin_fmaf(e2, e2, a[2]);
                        a[3] = __builtin_fmaf(e3, e3, a[3]);
                    }
                }
            } else {
                for (int f = 0; f < d; ++f) {
                    const float x = Xt[(long)f * ldx + ic];
                    const float4 cv = *reinterpret_cast<const float4*>(&Cs[f * KC + cc]);
                    const float e0 = x - cv.x, e1 = x - cv.y, e2 = x - cv.z, e3 = x - cv.w;
                    a[0] = __builtin_fmaf(e0, e0, a[0]);
                    a[1] = __builtin_fmaf(e1, e1, a[1]);
                    a[2] = __builtin_fmaf(e2, e2, a[2]);
                    a[3] = __builtin_fmaf(e3, e3, a[3]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = c0 + cc + u;
                const float w = a[u];
                if (valid && cc + u < kc && j != i && w < kth) {
                    int p = K - 1;                              // shift everything STRICTLY greater one place down
                    while (p > 0) {
                        const float t = Ld[(p - 1) * rows + tid];
                        if (!(t > w)) break;
                        Ld[p * rows + tid] = t;
                        Li[p * rows + tid] = Li[(p - 1) * rows + tid];
                        --p;
                    }
                    Ld[p * rows + tid] = w;
                    Li[p * rows + tid] = j;
                    kth = Ld[(K - 1) * rows + tid];
                }
            }
        }
    }
    if (valid) {
        for (int p = 0; p < K; ++p) {
            idx[(long)i * K + p] = Li[p * rows + tid];
            d2o[(long)i * K + p] = Ld[p * rows + tid];
        }
    }
}

// the 256 values of a workgroup in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double tsne_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = TSNE_TILE / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

template <bool MASK>
__device__ __forceinline__ void tsne_rep_tile(const float* __restrict__ xs, const float* __restrict__ ys, int kc4, int c0,
                                              int i, int N, float xi, float yi, float (&rx)[4], float (&ry)[4], float (&z)[4]) {
    for (int cc = 0; cc < kc4; cc += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(&xs[cc]);
        const float4 yv = *reinterpret_cast<const float4*>(&ys[cc]);
        const float xj[4] = {xv.x, xv.y, xv.z, xv.w}, yj[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float dx = xi - xj[u], dy = yi - yj[u];
            const float s = __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, 1.f));
            float q = __builtin_amdgcn_rcpf(s);
            if (MASK) q = (c0 + cc + u == i || c0 + cc + u >= N) ? 0.f : q;
            const float q2 = q * q;
            rx[u] = __builtin_fmaf(q2, dx, rx[u]);
            ry[u] = __builtin_fmaf(q2, dy, ry[u]);
            z[u] += q;
        }
    }
}

// grid (RT, S).  part [S][3][N]: rep_x, rep_y and sum of q of row i over the columns of range s.  The columns behind N in
// the last tile are staged as 0 and masked by index like j == i.
__global__ __launch_bounds__(TSNE_TILE) void tsne_repulsion_kernel(const float* __restrict__ Yt, long ldy,
                                                                   float* __restrict__ part, int N, TsnePlan pl, int vec) {
    __shared__ __attribute__((aligned(16))) float xs[TSNE_KC];
    __shared__ __attribute__((aligned(16))) float ys[TSNE_KC];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * TSNE_TILE, i = r0 + tid;
    const int ic = i < N ? i : N - 1;
    const float xi = Yt[ic], yi = Yt[ldy + ic];
    float rx[4] = {0.f, 0.f, 0.f, 0.f}, ry[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
    const int t0 = blockIdx.y * pl.tps, t1 = (t0 + pl.tps < pl.nct) ? t0 + pl.tps : pl.nct;
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * TSNE_KC;
        const int kc = (N - c0 < TSNE_KC) ? N - c0 : TSNE_KC;
        __syncthreads();
        if (vec) {
            if (tid < TSNE_KC / 4) {
                const int c4 = tid << 2;                        // N is not a multiple of 4 in general: per element
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (c4 + 3 < kc) {
                    a = *reinterpret_cast<const float4*>(Yt + c0 + c4);
                    b = *reinterpret_cast<const float4*>(Yt + ldy + c0 + c4);
                } else {
                    if (c4 < kc) { a.x = Yt[c0 + c4]; b.x = Yt[ldy + c0 + c4]; }
                    if (c4 + 1 < kc) { a.y = Yt[c0 + c4 + 1]; b.y = Yt[ldy + c0 + c4 + 1]; }
                    if (c4 + 2 < kc) { a.z = Yt[c0 + c4 + 2]; b.z = Yt[ldy + c0 + c4 + 2]; }
                }
                *reinterpret_cast<float4*>(&xs[c4]) = a;
                *reinterpret_cast<float4*>(&ys[c4]) = b;
            }
        } else {
            for (int cc = tid; cc < TSNE_KC; cc += TSNE_TILE) {
                xs[cc] = (cc < kc) ? Yt[c0 + cc] : 0.f;
                ys[cc] = (cc < kc) ? Yt[ldy + c0 + cc] : 0.f;
            }
        }
        __syncthreads();
        const int kc4 = (kc + 3) & ~3;
        if ((c0 < r0 + TSNE_TILE && c0 + kc > r0) || kc < TSNE_KC)
            tsne_rep_tile<true>(xs, ys, kc4, c0, i, N, xi, yi, rx, ry, z);
        else
            tsne_rep_tile<false>(xs, ys, kc4, c0, i, N, xi, yi, rx, ry, z);
    }
    if (i < N) {
        float* p = part + (long)blockIdx.y * 3 * N;
        p[i] = (rx[0] + rx[1]) + (rx[2] + rx[3]);
        p[(long)N + i] = (ry[0] + ry[1]) + (ry[2] + ry[3]);
        p[2L * N + i] = (z[0] + z[1]) + (z[2] + z[3]);
    }
}

// grid RT.  rep [2][ldy]; zpart[RT] = sum of the rows' z of the workgroup.
__global__ __launch_bounds__(TSNE_TILE) void tsne_rows_kernel(const float* __restrict__ part, float* __restrict__ rep,
                                                              long ldy, double* __restrict__ zpart, int N, int S) {
    __shared__ double red[TSNE_TILE];
    const int i = blockIdx.x * TSNE_TILE + threadIdx.x;
    double z = 0.0;
    if (i < N) {
        float rx = 0.f, ry = 0.f;
        for (int s = 0; s < S; ++s) {
            const float* p = part + (long)s * 3 * N;
            rx += p[i];
            ry += p[(long)N + i];
            z += (double)p[2L * N + i];
        }
        rep[i] = rx;
        rep[ldy + i] = ry;
    }
    const double tot = tsne_block_sum(z, red);
    if (threadIdx.x == 0) zpart[blockIdx.x] = tot;
}

// ONE workgroup: out[0] = sum of part[0 .. n)
__global__ __launch_bounds__(TSNE_TILE) void tsne_sum_kernel(const double* __restrict__ part, int n,
                                                             double* __restrict__ out) {
    __shared__ double red[TSNE_TILE];
    double v = 0.0;
    for (int g = threadIdx.x; g < n; g += TSNE_TILE) v += part[g];
    const double tot = tsne_block_sum(v, red);
    if (threadIdx.x == 0) out[0] = tot;
}

// grid RT.  Entries outside [0, nnz) and columns outside [0, N) are never read (a damaged CSR gives a wrong sum, not a
// wild access).
__global__ __launch_bounds__(TSNE_TILE) void tsne_step_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val, int nnz,
    const float* __restrict__ Yt, const float* __restrict__ rep, const double* __restrict__ Z, float* __restrict__ gains,
    float* __restrict__ update, float* __restrict__ Yo, float* __restrict__ grad_out, double* __restrict__ gpart, long ldy,
    int N, float alpha, float momentum, float lr) {
    __shared__ double red[TSNE_TILE];
    const int i = blockIdx.x * TSNE_TILE + threadIdx.x;
    double g2 = 0.0;
    if (i < N) {
        const float xi = Yt[i], yi = Yt[ldy + i];
        int e0 = rowptr[i], e1 = rowptr[i + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > nnz ? nnz : e1;
        float ax = 0.f, ay = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int j = col[e];
            if ((unsigned)j >= (unsigned)N) continue;
            const float dx = xi - Yt[j], dy = yi - Yt[ldy + j];
            const float pq = val[e] * __builtin_amdgcn_rcpf(__builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, 1.f)));
            ax = __builtin_fmaf(pq, dx, ax);
            ay = __builtin_fmaf(pq, dy, ay);
        }
        const float invz = (float)(1.0 / Z[0]);
        const float g[2] = {4.f * (alpha * ax - rep[i] * invz), 4.f * (alpha * ay - rep[ldy + i] * invz)};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const long o = c * ldy + i;
            const float u = update[o];
            float gn = gains[o];
            gn = (u * g[c] < 0.f) ? gn + 0.2f : gn * 0.8f;
            gn = gn < 0.01f ? 0.01f : gn;
            const float un = momentum * u - lr * gn * g[c];
            gains[o] = gn;
            update[o] = un;
            Yo[o] = Yt[o] + un;
            if (grad_out) grad_out[o] = g[c];
        }
        g2 = (double)g[0] * g[0] + (double)g[1] * g[1];
    }
    const double tot = tsne_block_sum(g2, red);
    if (threadIdx.x == 0) gpart[blockIdx.x] = tot;
}

// grid RT.  klpart[RT]
__global__ __launch_bounds__(TSNE_TILE) void tsne_kl_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                            const float* __restrict__ val, int nnz,
                                                            const float* __restrict__ Yt, long ldy,
                                                            const double* __restrict__ Z, double* __restrict__ klpart,
                                                            int N) {
    __shared__ double red[TSNE_TILE];
    const int i = blockIdx.x * TSNE_TILE + threadIdx.x;
    const double eps = 2.220446049250313e-16;
    double kl = 0.0;
    if (i < N) {
        const double xi = Yt[i], yi = Yt[ldy + i], z = Z[0];
        int e0 = rowptr[i], e1 = rowptr[i + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > nnz ? nnz : e1;
        for (int e = e0; e < e1; ++e) {
            const int j = col[e];
            if ((unsigned)j >= (unsigned)N) continue;
            const double dx = xi - (double)Yt[j], dy = yi - (double)Yt[ldy + j];
            const double q = 1.0 / (1.0 + dx * dx + dy * dy) / z;
            const double p = val[e];
            kl += p * log(fmax(p, eps) / fmax(q, eps));
        }
    }
    const double tot = tsne_block_sum(kl, red);
    if (threadIdx.x == 0) klpart[blockIdx.x] = tot;
}

}  // namespace tvae_cluster
