// Ward agglomerative clustering without an N x N matrix (libtvae_cluster.so).  Live centroids feature-major Ct[d][ldc]
// (the fp32 rounding of the fp64 centroids that the merge keeps), sizes cnt[M] as fp32.  One round = nearest neighbour
// of every live cluster under
//     w(i,j) = (cnt_i * cnt_j) / (cnt_i + cnt_j) * sum_f (c_if - c_jf)^2          (fp32, FMA chain in ascending f)
// then one merge of every reciprocal pair (Ward is reducible: reciprocal nearest neighbours belong to the dendrogram).
//
// ward_nn_kernel     a workgroup owns 256 rows (a thread = a row, its features in registers for d <= DREG) and a range
//                    of column tiles, which stream through LDS feature-major (four neighbouring columns = one 16-byte
//                    broadcast read).  w is bitwise symmetric: (x - y)^2 == (y - x)^2, and the size factor only uses
//                    commutative operations on (cnt_i, cnt_j).  Strict `<` in ascending j: ties go to the lowest j.
// ward_nn_reduce     the S column ranges of a row in ascending order, strict `<` again.  S depends on (M, d) only.
// ward_scan_kernel   ONE workgroup: exclusive prefix sums over the slots -> compacted position of every survivor and the
//                    rank of every merging pair (by ascending lower slot).  No atomics on positions.
// ward_apply_kernel  writes survivors / merged clusters into the second set of arrays and the merge records.
// No float atomics anywhere: every output is a pure function of the inputs.
#pragma once
#include <hip/hip_runtime.h>

namespace tvae_cluster {

constexpr int WARD_TILE = 256;           // rows per workgroup = threads per workgroup
constexpr int WARD_LDS_FLOATS = 8192;    // LDS budget of a column tile (32 KB: four workgroups per CU)
constexpr int WARD_KC_MAX = 256;         // columns per tile at most (small tiles = more column ranges for a small M)
constexpr int WARD_WGS = 2048;           // workgroups a launch aims at (8 per CU)
constexpr int WARD_SCAN = 1024;          // threads of the scan workgroup
constexpr int WARD_M_MAX = 1 << 24;      // sizes are exact in fp32 up to here
constexpr int WARD_FY = 8;               // feature slices (grid y) of the apply kernel

struct WardPlan {
    int RT, KC, nct, S, tps;             // row tiles, columns per tile, column tiles, column ranges, tiles per range
};

static inline WardPlan ward_plan(int M, int d) {
    WardPlan p;
    p.RT = (M + WARD_TILE - 1) / WARD_TILE;
    const int KC = (WARD_LDS_FLOATS / (d + 1)) & ~3;
    p.KC = KC < WARD_KC_MAX ? KC : WARD_KC_MAX;
    p.nct = (M + p.KC - 1) / p.KC;
    int want = WARD_WGS / p.RT;
    if (want < 1) want = 1;
    const int S = want < p.nct ? want : p.nct;
    p.tps = (p.nct + S - 1) / S;
    p.S = (p.nct + p.tps - 1) / p.tps;
    return p;
}

// every operation rounded on its own (no contraction), commutative in (ni, nj)
__device__ __forceinline__ float ward_w(float ni, float nj, float a) {
    return __fmul_rn(__fdiv_rn(__fmul_rn(ni, nj), __fadd_rn(ni, nj)), a);
}

// grid (RT, S).  pd / pj [S][M]: minimum and argmin of row i over the columns of range s (pj = -1: no column j != i)
template <int DREG>
__global__ __launch_bounds__(WARD_TILE) void ward_nn_kernel(const float* __restrict__ Ct, long ldc,
                                                            const float* __restrict__ cnt, float* __restrict__ pd,
                                                            int* __restrict__ pj, int M, int d, WardPlan pl, int vec) {
    extern __shared__ __attribute__((aligned(16))) float4 ward_s4[];
    float* Cs = reinterpret_cast<float*>(ward_s4);              // [d][KC]
    const int KC = pl.KC, tid = threadIdx.x;
    float* ns = Cs + d * KC;                                    // [KC] (d * KC is a multiple of 4)
    const int i = blockIdx.x * WARD_TILE + tid;
    const bool valid = i < M;
    const int ic = valid ? i : M - 1;
    float xr[DREG > 0 ? DREG : 1];
    if (DREG > 0) {
#pragma unroll
        for (int f = 0; f < DREG; ++f) xr[f] = (f < d) ? Ct[(long)f * ldc + ic] : 0.f;
    }
    const float ni = cnt[ic];
    float best = __builtin_inff();
    int bj = -1;
    const int t0 = blockIdx.y * pl.tps, t1 = (t0 + pl.tps < pl.nct) ? t0 + pl.tps : pl.nct;
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * KC;
        const int kc = (M - c0 < KC) ? M - c0 : KC;
        __syncthreads();
        if (vec) {                                              // c0 % 4 == 0, ldc % 4 == 0: a quad never leaves its row
            const int K4 = KC >> 2;
            for (int q = tid; q < d * K4; q += WARD_TILE) {
                const int f = q / K4, c4 = (q - f * K4) << 2;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c4 < kc) v = *reinterpret_cast<const float4*>(Ct + (long)f * ldc + c0 + c4);
                *reinterpret_cast<float4*>(&Cs[f * KC + c4]) = v;
            }
        } else {
            for (int q = tid; q < d * KC; q += WARD_TILE) {
                const int f = q / KC, cc = q - f * KC;
                Cs[f * KC + cc] = (cc < kc) ? Ct[(long)f * ldc + c0 + cc] : 0.f;
            }
        }
        for (int cc = tid; cc < KC; cc += WARD_TILE) ns[cc] = (cc < kc) ? cnt[c0 + cc] : 1.f;
        __syncthreads();
        for (int cc = 0; cc < kc; cc += 4) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            if (DREG > 0) {
#pragma unroll
                for (int f = 0; f < DREG; ++f) {
                    if (f < d) {
                        const float4 cv = *reinterpret_cast<const float4*>(&Cs[f * KC + cc]);
                        const float e0 = xr[f] - cv.x, e1 = xr[f] - cv.y, e2 = xr[f] - cv.z, e3 = xr[f] - cv.w;
                        a0 = __builtin_fmaf(e0, e0, a0);
                        a1 = __builtin_fmaf(e1, e1, a1);
                        a2 = __builtin_fmaf(e2, e2, a2);
                        a3 = __builtin_fmaf(e3, e3, a3);
                    }
                }
            } else {
                for (int f = 0; f < d; ++f) {
                    const float x = Ct[(long)f * ldc + ic];
                    const float4 cv = *reinterpret_cast<const float4*>(&Cs[f * KC + cc]);
                    const float e0 = x - cv.x, e1 = x - cv.y, e2 = x - cv.z, e3 = x - cv.w;
                    a0 = __builtin_fmaf(e0, e0, a0);
                    a1 = __builtin_fmaf(e1, e1, a1);
                    a2 = __builtin_fmaf(e2, e2, a2);
                    a3 = __builtin_fmaf(e3, e3, a3);
                }
            }
            const float4 nv = *reinterpret_cast<const float4*>(&ns[cc]);
            const float w0 = ward_w(ni, nv.x, a0), w1 = ward_w(ni, nv.y, a1);
            const float w2 = ward_w(ni, nv.z, a2), w3 = ward_w(ni, nv.w, a3);
            const int j = c0 + cc;
            if (j != i && w0 < best) { best = w0; bj = j; }
            if (cc + 1 < kc && j + 1 != i && w1 < best) { best = w1; bj = j + 1; }
            if (cc + 2 < kc && j + 2 != i && w2 < best) { best = w2; bj = j + 2; }
            if (cc + 3 < kc && j + 3 != i && w3 < best) { best = w3; bj = j + 3; }
        }
    }
    if (valid) {
        pd[(long)blockIdx.y * M + i] = best;
        pj[(long)blockIdx.y * M + i] = bj;
    }
}

// the S column ranges in ascending order.  A row whose every w is +inf or NaN still names a valid neighbour (the lowest
// j != i), so that nn is always an index.
__global__ __launch_bounds__(WARD_TILE) void ward_nn_reduce_kernel(const float* __restrict__ pd, const int* __restrict__ pj,
                                                                   int* __restrict__ nn, float* __restrict__ nd, int M,
                                                                   int S) {
    const int i = blockIdx.x * WARD_TILE + threadIdx.x;
    if (i >= M) return;
    float best = __builtin_inff();
    int bj = (i == 0) ? 1 : 0;
    for (int s = 0; s < S; ++s) {
        const float w = pd[(long)s * M + i];
        if (w < best) {                                         // (w < inf implies pj >= 0)
            best = w;
            bj = pj[(long)s * M + i];
        }
    }
    nn[i] = bj;
    nd[i] = best;
}

// One workgroup.  pos[i] = compacted slot of i (-1: absorbed into its partner), rank[i] = rank of the pair whose lower
// slot is i (-1: no pair or the upper slot); *m_out = number of survivors.
__global__ __launch_bounds__(WARD_SCAN) void ward_scan_kernel(const int* __restrict__ nn, int* __restrict__ pos,
                                                              int* __restrict__ rank, int* __restrict__ m_out, int M) {
    __shared__ int wsum[WARD_SCAN / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base_p = 0, base_r = 0;
    for (int c0 = 0; c0 < M; c0 += WARD_SCAN) {
        const int i = c0 + tid;
        int lead = 0, keep = 0;
        if (i < M) {
            const int j = nn[i];
            const bool mutual = j >= 0 && j < M && j != i && nn[j] == i;
            lead = mutual && i < j;
            keep = !mutual || i < j;
        }
        const int v = (lead << 16) | keep;                      // both counts of a 1024-slot chunk fit 16 bits
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < WARD_SCAN / 64; ++w) {
            const int s = wsum[w];
            if (w < wv) off += s;
            tot += s;
        }
        __syncthreads();
        const int excl = off + incl - v;
        if (i < M) {
            pos[i] = keep ? base_p + (excl & 0xffff) : -1;
            rank[i] = lead ? base_r + (excl >> 16) : -1;
        }
        base_p += tot & 0xffff;
        base_r += tot >> 16;
    }
    if (tid == 0) *m_out = base_p;
}

// grid (M / 256, min(d, WARD_FY)): a thread = an old slot, the y index strides the features; slice 0 also writes the
// per-slot scalars and the merge record.  Centroids live in fp64 (C64) and the search reads their fp32 rounding (Co):
// the centroid of a merged cluster does not inherit one fp32 rounding per level of the tree, and the recorded height is
// the fp64 Ward distance of the pair, so two merges whose heights differ by less than an fp32 ulp still sort as they
// do in an fp64 reference.
__global__ __launch_bounds__(WARD_TILE) void ward_apply_kernel(
    const double* __restrict__ Ci, long ldi, const float* __restrict__ cnt_i, const int* __restrict__ id_i,
    const double* __restrict__ hmax_i, const int* __restrict__ nn, const int* __restrict__ pos,
    const int* __restrict__ rank, double* __restrict__ Co64, float* __restrict__ Co, long ldo, float* __restrict__ cnt_o,
    int* __restrict__ id_o, double* __restrict__ hmax_o, int* __restrict__ rec_ids, double* __restrict__ rec_hs, int M,
    int d, int N, int base, int cap) {
    const int i = blockIdx.x * WARD_TILE + threadIdx.x;
    if (i >= M) return;
    const int p = pos[i];
    if (p < 0) return;
    const int r = rank[i], f0 = blockIdx.y, fs = gridDim.y;
    if (r < 0) {
        for (int f = f0; f < d; f += fs) {
            const double c = Ci[(long)f * ldi + i];
            Co64[(long)f * ldo + p] = c;
            Co[(long)f * ldo + p] = (float)c;
        }
        if (f0 == 0) {
            cnt_o[p] = cnt_i[i];
            id_o[p] = id_i[i];
            hmax_o[p] = hmax_i[i];
        }
        return;
    }
    const int j = nn[i];
    const float ni = cnt_i[i], nj = cnt_i[j], nsum = __fadd_rn(ni, nj);       // exact integers
    const double di = ni, dj = nj, ds = nsum;
    for (int f = f0; f < d; f += fs) {
        const double c = (di * Ci[(long)f * ldi + i] + dj * Ci[(long)f * ldi + j]) / ds;
        Co64[(long)f * ldo + p] = c;
        Co[(long)f * ldo + p] = (float)c;
    }
    if (f0 == 0) {
        double a = 0.0;
        for (int f = 0; f < d; ++f) {
            const double e = Ci[(long)f * ldi + i] - Ci[(long)f * ldi + j];
            a = __builtin_fma(e, e, a);
        }
        const double h = fmax(fmax(sqrt(2.0 * (di * dj / ds) * a), hmax_i[i]), hmax_i[j]);
        const int q = base + r;
        if (q < cap) {
            rec_ids[2 * (long)q] = id_i[i];
            rec_ids[2 * (long)q + 1] = id_i[j];
            rec_hs[2 * (long)q] = h;
            rec_hs[2 * (long)q + 1] = ds;
        }
        cnt_o[p] = nsum;
        id_o[p] = N + q;
        hmax_o[p] = h;
    }
}

}  // namespace tvae_cluster
