// Quality measures of the aligned class averages (libtvae_cluster.so): in the single pass over the stack that
// avg_accum_kernel makes, the two half-set averages and the per-pixel variance of every class, and from two stacks of
// planes the Fourier ring correlation.  Included by abi_align.hip only (align_sample and avg_seg_kernel come from
// align_kernels.hpp, which exactly one unit may see).
//
// halves_accum_kernel   avg_accum_kernel with three accumulators: a workgroup = 256 pixels x one channel x one chunk of a
//                       class.  A chunk starts at a multiple of AVG_CHUNK (even) counted from the class's first position, so
//                       the parity of a member's index within its chunk is the parity of its position in the class: even
//                       members go to S0, odd ones to S1 and the square of every sample (taken ONCE, squared from the
//                       register) to Q.  The member loop runs over PAIRS: no branch on the parity, a missing last member is a
//                       sample with on = false, an exact 0.  fp32 sums in ascending position, as the header states.
// halves_reduce_kernel  a thread = a pixel of class k, channel ch: the class's slots in ascending order in fp64, then the two
//                       half averages, the average and the variance, each rounded to fp32 once.
// frc_rows_kernel       stage 1 of the direct 2-D DFT: a workgroup = FRC_ROWS rows of one plane of `a` or of `b`.  The rows are
//                       read contiguously, multiplied by the mask and kept in LDS beside the n twiddles; a thread = one
//                       (row, kx), kx = 0 .. n / 2, and walks j with the table index (kx j) mod n kept in integers.
// frc_cols_kernel       stage 2: a thread = one kx and FRC_KY consecutive ky of one plane, lanes along kx (the half spectra of
//                       stage 1 are read coalesced, once per FRC_KY outputs), both `a` and `b`, so that what goes back to the
//                       workspace is the three products of a coefficient, not the coefficients.
// frc_rings_kernel      a thread = one ring of one plane.  For a given ky the kx of a ring form one interval, found in exact
//                       integer arithmetic; the thread walks ky in ascending index and kx in ascending order and adds in fp64
//                       with the Hermitian weights of the half spectrum.  A fixed order, no atomics.
// The twiddles cos and sin of 2 pi t / n are built once per workgroup (dft_twiddles of cluster_common.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "align_kernels.hpp"

namespace tvae_cluster {

constexpr int FRC_P_MAX = 65535;         // planes: the y dimension of the launch grids
constexpr int FRC_ROWS = 8;              // rows of a plane per workgroup of stage 1
constexpr int FRC_KY = 4;                // ky per thread of stage 2
constexpr int FRC_TILE = 256;            // threads per workgroup of stages 1 and 2
constexpr int FRC_RING_TILE = 64;        // threads (rings) per workgroup of the ring sums

// floats of workspace per plane: the half spectra of the rows of a and b (complex) and the three products per coefficient
static inline long frc_plane_floats(int n) { return 7L * n * half_side(n); }

// grid = slots * C * tiles (tile fastest, then channel).  part[slots][C][3][n][n] (S0, S1, Q), cnt[slots][2] (written by
// tile 0 of channel 0)
__global__ __launch_bounds__(ALIGN_TILE) void halves_accum_kernel(const float* __restrict__ Y,
                                                                  const float* __restrict__ theta,
                                                                  const float* __restrict__ dx,
                                                                  const int* __restrict__ order,
                                                                  const int* __restrict__ clean, float* __restrict__ part,
                                                                  int* __restrict__ cnt, int N, int C, int n, int K,
                                                                  int tiles, float t_scale) {
    __shared__ AlignPose pose[AVG_CHUNK];
    __shared__ int member[AVG_CHUNK];
    AvgChunk w;
    if (!w.load(blockIdx.x, clean, order, theta, dx, N, C, K, tiles, t_scale, pose, member)) return;
    const int tile = w.tile, ch = w.ch, slot = w.slot, members = w.members;
    if (tile == 0 && ch == 0 && threadIdx.x < 2) {
        int v = 0;
        for (int m = threadIdx.x; m < members; m += 2) v += member[m] >= 0;
        cnt[2 * slot + threadIdx.x] = v;
    }
    const int p = tile * ALIGN_TILE + threadIdx.x;
    if (p >= n * n) return;
    const int i = p / n, j = p % n;
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const size_t nn = (size_t)n * n;
    float s0 = 0.f, s1 = 0.f, q = 0.f;
    const int pairs = (members + 1) >> 1;                     // member[members] = -1 where `members` is odd
#pragma unroll 2
    for (int m = 0; m < pairs; ++m) {
        const int id0 = member[2 * m], id1 = member[2 * m + 1];
        const bool on0 = id0 >= 0, on1 = id1 >= 0;
        const float a0 = align_sample(Y + ((size_t)(on0 ? id0 : 0) * C + ch) * nn, n, i, j, step, half, pose[2 * m], on0);
        const float a1 = align_sample(Y + ((size_t)(on1 ? id1 : 0) * C + ch) * nn, n, i, j, step, half, pose[2 * m + 1],
                                      on1);
        s0 += a0;
        s1 += a1;
        q = fmaf(a0, a0, q);
        q = fmaf(a1, a1, q);
    }
    float* dst = part + ((size_t)slot * C + ch) * 3 * nn + p;
    dst[0] = s0;
    dst[nn] = s1;
    dst[2 * nn] = q;
}

// grid = K * C * tiles (tile fastest).  avg[K][C][n][n], half[2][K][C][n][n], var[K][C][n][n], counts[K][2]
__global__ __launch_bounds__(ALIGN_TILE) void halves_reduce_kernel(const float* __restrict__ part,
                                                                   const int* __restrict__ cnt,
                                                                   const int* __restrict__ clean, float* __restrict__ avg,
                                                                   float* __restrict__ half, float* __restrict__ var,
                                                                   int* __restrict__ counts, int K, int C, int n,
                                                                   int tiles) {
    const int tile = blockIdx.x % tiles;
    const long plane = blockIdx.x / tiles;                    // class * C + channel
    const int k = (int)(plane / C), ch = (int)(plane % C);
    const int p = tile * ALIGN_TILE + threadIdx.x;
    const int sk = clean[k], ek = clean[k + 1];
    const int chunks = (ek - sk + AVG_CHUNK - 1) / AVG_CHUNK;
    const int slot0 = sk / AVG_CHUNK + k;
    int n0 = 0, n1 = 0;
    for (int c = 0; c < chunks; ++c) {
        n0 += cnt[2 * (slot0 + c)];
        n1 += cnt[2 * (slot0 + c) + 1];
    }
    if (tile == 0 && ch == 0 && threadIdx.x == 0) {
        counts[2 * k] = n0;
        counts[2 * k + 1] = n1;
    }
    if (p >= n * n) return;
    const size_t nn = (size_t)n * n;
    double s0 = 0.0, s1 = 0.0, q = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const float* src = part + ((size_t)(slot0 + c) * C + ch) * 3 * nn + p;
        s0 += (double)src[0];
        s1 += (double)src[nn];
        q += (double)src[2 * nn];
    }
    const int m = n0 + n1;
    const double s = s0 + s1;
    const size_t at = (size_t)plane * nn + p, kcnn = (size_t)K * C * nn;
    half[at] = n0 > 0 ? (float)(s0 / (double)n0) : 0.f;
    half[kcnn + at] = n1 > 0 ? (float)(s1 / (double)n1) : 0.f;
    avg[at] = m > 0 ? (float)(s / (double)m) : 0.f;
    float v = 0.f;
    if (m >= 2) {
        const double d = (q - s * s / (double)m) / (double)(m - 1);
        v = (float)(d < 0.0 ? 0.0 : d);                       // (a NaN stays a NaN)
    }
    var[at] = v;
}

// (frc_mask, the mask m(i, j), and frc_first_kx, the kx interval of a ring: cluster_common.hpp, shared with the ring power)

// grid = (ceil(n / FRC_ROWS), P, 2): z = 0 reads a, z = 1 reads b.  G[P][2][n][H] complex, H = n / 2 + 1:
// G(i, kx) = sum_j x[i][j] m(i, j) exp(-2 pi i kx j / n)
__global__ __launch_bounds__(FRC_TILE) void frc_rows_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float2* __restrict__ G, int n, float radius, float edge) {
    __shared__ float2 tw[SIDE_MAX];
    __shared__ float row[FRC_ROWS * SIDE_MAX];
    const int H = half_side(n);
    const int i0 = blockIdx.x * FRC_ROWS;
    const int rows = min(FRC_ROWS, n - i0);
    const size_t plane = blockIdx.y;
    const float* __restrict__ x = (blockIdx.z == 0 ? a : b) + (plane * n + i0) * n;
    dft_twiddles(tw, n, blockDim.x);
    for (int e = threadIdx.x; e < rows * n; e += FRC_TILE) {  // the rows are adjacent in memory: one contiguous read
        const int r = e / n, j = e - r * n;
        row[r * n + j] = x[e] * frc_mask(i0 + r, j, n, radius, edge);
    }
    __syncthreads();
    float2* __restrict__ dst = G + ((plane * 2 + blockIdx.z) * n + i0) * H;
    for (int e = threadIdx.x; e < rows * H; e += FRC_TILE) {
        const int r = e / H, kx = e - r * H;
        const float* __restrict__ xr = row + r * n;
        float re = 0.f, im = 0.f;
        int t = 0;                                            // (kx j) mod n
        for (int j = 0; j < n; ++j) {
            const float2 w = tw[t];
            const float v = xr[j];
            re = fmaf(v, w.x, re);
            im = fmaf(-v, w.y, im);
            tw_advance(t, kx, n);
        }
        dst[e] = make_float2(re, im);                         // e = r * H + kx: the rows of G are adjacent as well
    }
}

// grid = (ceil(ceil(n / FRC_KY) * H / FRC_TILE), P).  prod[P][3][n][H]: Re(Fa conj Fb), |Fa|^2, |Fb|^2 at (ky, kx) with
// F(ky, kx) = sum_i G(i, kx) exp(-2 pi i ky i / n); the products in fp64 from the fp32 coefficients, rounded to fp32 once
__global__ __launch_bounds__(FRC_TILE) void frc_cols_kernel(const float2* __restrict__ G, float* __restrict__ prod, int n) {
    __shared__ float2 tw[SIDE_MAX];
    const int H = half_side(n);
    const int groups = (n + FRC_KY - 1) / FRC_KY;
    const size_t plane = blockIdx.y;
    dft_twiddles(tw, n, blockDim.x);
    __syncthreads();
    const int e = blockIdx.x * FRC_TILE + threadIdx.x;
    if (e >= groups * H) return;
    const int g = e / H, kx = e - g * H;                      // lanes along kx
    const float2* __restrict__ ga = G + plane * 2 * n * H + kx;
    const float2* __restrict__ gb = ga + (size_t)n * H;
    int ky[FRC_KY], t[FRC_KY];
    float are[FRC_KY], aim[FRC_KY], bre[FRC_KY], bim[FRC_KY];
#pragma unroll
    for (int u = 0; u < FRC_KY; ++u) {
        ky[u] = min(g * FRC_KY + u, n - 1);                   // (a ky behind the end repeats the last one and is not stored)
        t[u] = 0;
        are[u] = aim[u] = bre[u] = bim[u] = 0.f;
    }
    for (int i = 0; i < n; ++i) {
        const float2 va = ga[(size_t)i * H], vb = gb[(size_t)i * H];
#pragma unroll
        for (int u = 0; u < FRC_KY; ++u) {
            const float2 w = tw[t[u]];                        // (c, s): v (c - i s)
            are[u] = fmaf(va.x, w.x, fmaf(va.y, w.y, are[u]));
            aim[u] = fmaf(va.y, w.x, fmaf(-va.x, w.y, aim[u]));
            bre[u] = fmaf(vb.x, w.x, fmaf(vb.y, w.y, bre[u]));
            bim[u] = fmaf(vb.y, w.x, fmaf(-vb.x, w.y, bim[u]));
            tw_advance(t[u], ky[u], n);
        }
    }
    float* __restrict__ dst = prod + plane * 3 * n * H + kx;
    const size_t nH = (size_t)n * H;
#pragma unroll
    for (int u = 0; u < FRC_KY; ++u) {
        if (g * FRC_KY + u >= n) continue;
        const double ar = are[u], ai = aim[u], br = bre[u], bi = bim[u];
        const size_t at = (size_t)ky[u] * H;
        dst[at] = (float)(ar * br + ai * bi);
        dst[nH + at] = (float)(ar * ar + ai * ai);
        dst[2 * nH + at] = (float)(br * br + bi * bi);
    }
}

// grid = (ceil(R / FRC_RING_TILE), P), R = n / 2 + 1.  sums[P][R][3] (fp64), frc[P][R].  Ring r holds the (ky, kx) with
// r - 1/2 <= sqrt(ky^2 + kx^2) < r + 1/2, in integers (2r - 1)^2 <= 4 (ky^2 + kx^2) < (2r + 1)^2 (the lower test is empty for
// r = 0).  The half spectrum kx = 0 .. n / 2 stands for the full plane: a coefficient with 0 < kx < n / 2 (and kx = n / 2 of an
// odd n does not exist) counts twice, once for its mirror image (-ky, -kx), whose three products are the same.
__global__ __launch_bounds__(FRC_RING_TILE) void frc_rings_kernel(const float* __restrict__ prod, float* __restrict__ frc,
                                                                  double* __restrict__ sums, int n) {
    const int H = half_side(n);
    const int r = blockIdx.x * FRC_RING_TILE + threadIdx.x;
    if (r >= H) return;
    const size_t plane = blockIdx.y;
    const size_t nH = (size_t)n * H;
    const float* __restrict__ src = prod + plane * 3 * nH;
    const int lo2 = (2 * r - 1) * (2 * r - 1), hi2 = (2 * r + 1) * (2 * r + 1);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int row = 0; row < n; ++row) {                       // numpy's fftfreq order: 0, 1, ..., then the negative ones
        const int ky = row < (n + 1) / 2 ? row : row - n;
        const int k4 = 4 * ky * ky;
        const int a = r == 0 ? 0 : frc_first_kx(lo2 - k4);
        const int b = min(frc_first_kx(hi2 - k4), H);
        for (int kx = a; kx < b; ++kx) {
            const double w = (kx == 0 || 2 * kx == n) ? 1.0 : 2.0;
            const size_t at = (size_t)row * H + kx;
            s0 += w * (double)src[at];
            s1 += w * (double)src[nH + at];
            s2 += w * (double)src[2 * nH + at];
        }
    }
    double* __restrict__ out = sums + (plane * H + r) * 3;
    out[0] = s0;
    out[1] = s1;
    out[2] = s2;
    frc[plane * H + r] = (s1 == 0.0 || s2 == 0.0) ? 0.f : (float)(s0 / sqrt(s1 * s2));
}

}  // namespace tvae_cluster
