// Batched Lloyd k-means (libtvae_cluster.so).  Points feature-major Xt[d][ldx], centroids C[R][k][d].
//
// One workgroup = one (point group g, restart r): a contiguous range of 256-point tiles.
//   phase 1  a thread owns a point: distances in the direct form sum_j (x_j - c_j)^2 (fp32 FMA, ascending j) against the
//            centroids, which sit in LDS feature-major (four neighbouring centroids = one 16-byte broadcast read);
//            strict `<` in ascending cluster order: ties go to the lowest index.  Labels and mind2 go to HBM, the
//            per-cluster counts to an LDS histogram (integer atomics).
//   phase 2  threads switch roles and own (cluster, feature) pairs: they walk the group's points in order, labels as
//            LDS broadcasts, x as 16-byte loads along the point index, and add x where label == cluster, running
//            sums in registers over the whole tile range.  No float atomics: a sum is one thread's ordered chain.
// The update kernel adds the G partials in ascending g.  G depends on (N, d, k) only, so a restart's numbers do not
// depend on how many restarts share the launch.
#pragma once
#include <hip/hip_runtime.h>

namespace tvae_cluster {

constexpr int TILE = 256;            // points per tile = threads per workgroup
constexpr int PPT = 4;               // (cluster, feature) pairs a thread keeps in registers in phase 2
constexpr int CS_FLOATS = 8192;      // LDS budget of a centroid chunk (32 KB: four workgroups per CU)
constexpr int GROUPS_MAX = 64;
constexpr long GROUP_FLOATS_MAX = 1L << 22;   // partial sums per restart (16 MB) before G is cut down

struct Plan {
    int tiles, G, tpg, KC;
    long per_restart;                // floats of workspace per restart
};

static inline Plan make_plan(int N, int d, int k) {
    Plan p;
    p.tiles = (int)(((long)N + TILE - 1) / TILE);     // N may sit within a tile of 2^31
    long cap = GROUP_FLOATS_MAX / ((long)k * (d + 1));
    if (cap < 1) cap = 1;
    int G = p.tiles < GROUPS_MAX ? p.tiles : GROUPS_MAX;
    if (G > cap) G = (int)cap;
    p.tpg = (p.tiles + G - 1) / G;
    p.G = (p.tiles + p.tpg - 1) / p.tpg;
    const int k4 = (k + 3) & ~3;
    int KC = (CS_FLOATS / d) & ~3;
    p.KC = KC < k4 ? KC : k4;
    p.per_restart = (long)p.G * ((long)k * d + k + 2);
    return p;
}

__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = TILE / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ int block_sum_int(int v, int* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = TILE / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// DREG > 0: d <= DREG and the point's features stay in registers; DREG == 0: they are re-read (L1 / L2) per centroid group
template <int DREG>
__global__ __launch_bounds__(TILE) void kmeans_assign_kernel(const float* __restrict__ Xt, long ldx,
                                                             const float* __restrict__ C, const int* __restrict__ done,
                                                             int* labels, float* __restrict__ mind2, float* __restrict__ ws,
                                                             int N, int d, int k, Plan pl, int vec) {
    const int g = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    if (done[r]) return;
    extern __shared__ float4 cs4[];
    float* Cs = reinterpret_cast<float*>(cs4);                  // [d][KC]
    __shared__ __attribute__((aligned(16))) int lab_s[TILE];
    __shared__ int cnt_s[1024];
    __shared__ float red_f[TILE];
    __shared__ int red_i[TILE];

    const int KC = pl.KC, npairs = k * d;
    const float* Cr = C + (long)r * npairs;
    int* lab_r = labels + (long)r * N;
    float* md_r = mind2 + (long)r * N;
    float* wsr = ws + (long)r * pl.per_restart;
    float* sums = wsr + (long)g * npairs;
    int* counts = reinterpret_cast<int*>(wsr + (long)pl.G * npairs) + (long)g * k;
    int* chg_out = reinterpret_cast<int*>(wsr + (long)pl.G * npairs + (long)pl.G * k) + g;
    float* inert_out = wsr + (long)pl.G * npairs + (long)pl.G * k + pl.G + g;
    const int t0 = g * pl.tpg, t1 = (t0 + pl.tpg < pl.tiles) ? t0 + pl.tpg : pl.tiles;
    const int nchunks = (k + KC - 1) / KC;

    for (int c = tid; c < k; c += TILE) cnt_s[c] = 0;
    float inert = 0.f;
    int chg = 0;

    // ---- phase 1: labels ------------------------------------------------------------------------------------------------
    for (int t = t0; t < t1; ++t) {
        const long p = (long)t * TILE + tid;                    // the last tile may reach past 2^31
        const bool valid = p < N;
        const long pc = valid ? p : N - 1;
        float xr[DREG > 0 ? DREG : 1];
        if (DREG > 0) {
#pragma unroll
            for (int j = 0; j < DREG; ++j) xr[j] = (j < d) ? Xt[(long)j * ldx + pc] : 0.f;
        }
        float best = __builtin_inff();
        int bc = 0;
        for (int ch = 0; ch < nchunks; ++ch) {
            const int c0 = ch * KC;
            const int kc = (k - c0 < KC) ? k - c0 : KC;
            if (nchunks > 1 || t == t0) {
                __syncthreads();
                for (int q = tid; q < KC * d; q += TILE) {
                    const int cc = q / d, j = q - cc * d;
                    Cs[j * KC + cc] = (cc < kc) ? Cr[(long)(c0 + cc) * d + j] : 0.f;
                }
                __syncthreads();
            }
            for (int cc = 0; cc < kc; cc += 4) {
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                if (DREG > 0) {
#pragma unroll
                    for (int j = 0; j < DREG; ++j) {
                        if (j < d) {
                            const float4 cv = *reinterpret_cast<const float4*>(&Cs[j * KC + cc]);
                            const float e0 = xr[j] - cv.x, e1 = xr[j] - cv.y, e2 = xr[j] - cv.z, e3 = xr[j] - cv.w;
                            a0 = __builtin_fmaf(e0, e0, a0);
                            a1 = __builtin_fmaf(e1, e1, a1);
                            a2 = __builtin_fmaf(e2, e2, a2);
                            a3 = __builtin_fmaf(e3, e3, a3);
                        }
                    }
                } else {
                    for (int j = 0; j < d; ++j) {
                        const float x = Xt[(long)j * ldx + pc];
                        const float4 cv = *reinterpret_cast<const float4*>(&Cs[j * KC + cc]);
                        const float e0 = x - cv.x, e1 = x - cv.y, e2 = x - cv.z, e3 = x - cv.w;
                        a0 = __builtin_fmaf(e0, e0, a0);
                        a1 = __builtin_fmaf(e1, e1, a1);
                        a2 = __builtin_fmaf(e2, e2, a2);
                        a3 = __builtin_fmaf(e3, e3, a3);
                    }
                }
                if (a0 < best) { best = a0; bc = c0 + cc; }
                if (cc + 1 < kc && a1 < best) { best = a1; bc = c0 + cc + 1; }
                if (cc + 2 < kc && a2 < best) { best = a2; bc = c0 + cc + 2; }
                if (cc + 3 < kc && a3 < best) { best = a3; bc = c0 + cc + 3; }
            }
        }
        if (valid) {
            chg += (lab_r[p] != bc);
            lab_r[p] = bc;
            md_r[p] = best;
            inert += best;
            atomicAdd(&cnt_s[bc], 1);
        }
    }
    const float inert_wg = block_sum(inert, red_f, tid);
    const int chg_wg = block_sum_int(chg, red_i, tid);        // (its barriers also order cnt_s and this group's labels)
    for (int c = tid; c < k; c += TILE) counts[c] = cnt_s[c];
    if (tid == 0) {
        *chg_out = chg_wg;
        *inert_out = inert_wg;
    }

    // ---- phase 2: per-cluster sums of this group's points ----------------------------------------------------------------
    const int wave0 = tid & ~63;                                // pairs are skipped wave by wave (uniform branch)
    for (int q0 = 0; q0 < npairs; q0 += TILE * PPT) {
        int cq[PPT];
        long row[PPT];
        float s[PPT];
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int q = q0 + i * TILE + tid;
            const bool ok = q < npairs;
            const int c = ok ? q / d : 0;
            cq[i] = ok ? c : -2;
            row[i] = ok ? (long)(q - c * d) * ldx : 0;
            s[i] = 0.f;
        }
        for (int t = t0; t < t1; ++t) {
            const long base = (long)t * TILE;
            __syncthreads();
            lab_s[tid] = (base + tid < N) ? lab_r[base + tid] : -1;
            __syncthreads();
            if (vec && base + TILE <= N) {
                for (int pp = 0; pp < TILE; pp += 4) {
                    const int4 l = *reinterpret_cast<const int4*>(&lab_s[pp]);
#pragma unroll
                    for (int i = 0; i < PPT; ++i) {
                        if (q0 + i * TILE + wave0 < npairs) {
                            const float4 x = *reinterpret_cast<const float4*>(Xt + row[i] + base + pp);
                            s[i] += (l.x == cq[i]) ? x.x : 0.f;
                            s[i] += (l.y == cq[i]) ? x.y : 0.f;
                            s[i] += (l.z == cq[i]) ? x.z : 0.f;
                            s[i] += (l.w == cq[i]) ? x.w : 0.f;
                        }
                    }
                }
            } else {
                const int np = (N - base < TILE) ? (int)(N - base) : TILE;
                for (int pp = 0; pp < np; ++pp) {
                    const int l = lab_s[pp];
#pragma unroll
                    for (int i = 0; i < PPT; ++i) {
                        if (q0 + i * TILE + wave0 < npairs) {
                            const float x = Xt[row[i] + base + pp];
                            s[i] += (l == cq[i]) ? x : 0.f;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int q = q0 + i * TILE + tid;
            if (q < npairs) sums[q] = s[i];
        }
    }
}

// grid = R: the G partials of a restart in ascending g; empty clusters keep their centroid
__global__ __launch_bounds__(TILE) void kmeans_update_kernel(const float* __restrict__ ws, const int* __restrict__ done,
                                                             float* C, float* __restrict__ inertia,
                                                             float* __restrict__ shift, int d, int k, Plan pl) {
    const int r = blockIdx.x, tid = threadIdx.x;
    if (done[r]) return;
    __shared__ float red_f[TILE];
    const int npairs = k * d, G = pl.G;
    const float* wsr = ws + (long)r * pl.per_restart;
    const int* counts = reinterpret_cast<const int*>(wsr + (long)G * npairs);
    const float* inert = wsr + (long)G * npairs + (long)G * k + G;
    float* Cr = C + (long)r * npairs;
    float sh = 0.f;
    for (int q = tid; q < npairs; q += TILE) {
        const int c = q / d;
        int n = 0;
        for (int g = 0; g < G; ++g) n += counts[(long)g * k + c];
        if (n > 0) {
            float s = 0.f;
            for (int g = 0; g < G; ++g) s += wsr[(long)g * npairs + q];
            const float cn = s / (float)n, e = cn - Cr[q];
            sh = __builtin_fmaf(e, e, sh);
            Cr[q] = cn;
        }
    }
    const float sh_all = block_sum(sh, red_f, tid);
    if (tid == 0) {
        float it = 0.f;
        for (int g = 0; g < G; ++g) it += inert[g];
        inertia[r] = it;
        shift[r] = sh_all;
    }
}

// one thread per restart: changed[r] = sum of the groups' counts
__global__ __launch_bounds__(64) void kmeans_changed_sum_kernel(const float* __restrict__ ws, const int* __restrict__ done,
                                                                int* __restrict__ changed, int d, int k, int R, Plan pl) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R || done[r]) return;
    const int* chg = reinterpret_cast<const int*>(ws + (long)r * pl.per_restart + (long)pl.G * k * d + (long)pl.G * k);
    int n = 0;
    for (int g = 0; g < pl.G; ++g) n += chg[g];
    changed[r] = n;
}

// D[r][n] = min(D[r][n], ||x_n - cnew[r]||^2): grid (N / 256, R)
__global__ __launch_bounds__(TILE) void kmeans_mindist_kernel(const float* __restrict__ Xt, long ldx,
                                                              const float* __restrict__ cnew, float* __restrict__ D, int N,
                                                              int d) {
    const long p = (long)blockIdx.x * TILE + threadIdx.x;
    const int r = blockIdx.y;
    if (p >= N) return;
    const float* c = cnew + (long)r * d;
    float a = 0.f;
    for (int j = 0; j < d; ++j) {
        const float e = Xt[(long)j * ldx + p] - c[j];
        a = __builtin_fmaf(e, e, a);
    }
    float* o = D + (long)r * N + p;
    *o = fminf(*o, a);
}

}  // namespace tvae_cluster
