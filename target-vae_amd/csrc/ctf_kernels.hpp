// Per-image Fourier filtering with a real transfer function (include/tvae_cluster.h, last section): the CTF evaluated from five
// fp64 coefficients per image, the filter out = Re IDFT(H DFT(x)) of every plane of a stack, and the per-class sums of H^2.
//
// ctf_value             H(ky, kx) of one coefficient row.  q = (ks^2 + kx^2) / n^2 from the exact integer numerator (one fp64
//                       division), t = c2 q + c3 q^2 in fp64 and reduced to t - rint(t) there, sin and cos of 2 pi t by
//                       sincospi in fp64 on the exact argument 2 t, c0 sin + c1 cos in fp64 and rounded to fp32 ONCE, the
//                       envelope expf of the fp32 rounding of -c4 q (1 ulp, plus |c4 q| 2^-24 exp(-c4 q) <= 0.37 2^-24 from the
//                       argument for c4 q >= 0), one fp32 product: about 3 2^-24 (|c0| + |c1|), inside the contract's 8.
//                       Every kernel here calls this one function: an image's H is the same bits wherever it is formed.
// ctf_eval_kernel       a thread = one (ky, kx) of one row.
// ctf_filter_kernel     ONE 256-thread workgroup (four waves) owns ONE plane from load to store; a direct DFT in four stages
//                       on v_mfma_f32_32x32x2_f32 (the fragment layout: cluster_common.hpp):
//                         1 rows          G(i, kx)  = sum_j  x(i, j) e^{-2 pi i kx j / n}              2 MFMAs per k step
//                         2 columns       F(ky, kx) = sum_i  e^{-2 pi i ky i / n} G(i, kx)             4
//                           multiply      F *= H(ky, kx) w_kx, H formed in registers (or read from the caller's plane)
//                         3 columns back  P(i, kx)  = sum_ky e^{+2 pi i ky i / n} F(ky, kx)            4
//                         4 rows back     out(i, j) = n^-2 sum_kx Re(P(i, kx) e^{+2 pi i kx j / n})    2
//                       A wave walks 32 x 32 output tiles (tile = wave, wave + 4, ...), the whole reduction of a tile in its
//                       registers.  The twiddle operand of every stage is NOT staged: a lane reads it from the table of the n
//                       values (cos, sin)(2 pi t / n) at t = (a k) mod n, kept in integers (tw_advance by 2 a mod n per step), so
//                       no argument is ever reduced in floating point.  The data operand comes from one of two buffers of
//                       2 n ld floats (re plane, im plane; row stride ld = (n / 2 + 1) | 1, odd: the A-fragment reads of 32
//                       consecutive rows at a fixed k and the B-fragment reads of 32 consecutive columns are conflict-free):
//                       buffer 0 holds x (row stride n | 1), then F; buffer 1 holds G, then P.  Rows, columns and k outside
//                       the plane are PREDICATED zeros, never loaded, and nothing outside the plane is stored.
//                       Routes: ONDIE (n <= CTF_ONDIE_MAX = 128) keeps both buffers in LDS, 8 n + 16 n ld bytes (134 144 at
//                       n = 128: one workgroup per CU): in coefficient mode neither the spectrum nor H is ever in HBM.  Any
//                       larger n runs the SAME code on the plane's own 4 n ld floats of the caller's workspace (LDS holds the
//                       table only); a workgroup reads only what it wrote itself, behind workgroup barriers.
//                       The plane is read completely before the first barrier and written after the last: out may be X.
// ctf_power_kernel      a thread = one (ky, kx) of class k: the members in ascending position, H_i^2 formed and added in fp64.
//                       The cleaned boundaries min(max(0, seg[0 .. k]), N) of its class are found by the workgroup itself (a
//                       strided maximum and a fixed tree; a maximum does not depend on the order), the rule of avg_seg_kernel.
// No atomics anywhere; every output is a pure function of its own plane / class.
#pragma once
#include <hip/hip_runtime.h>

#include "cluster_common.hpp"

namespace tvae_cluster {

constexpr int CTF_THREADS = 256;
constexpr int CTF_ONDIE_MAX = 128;       // the largest n whose two buffers sit in LDS

__host__ __device__ static inline int ctf_ld(int n) { return half_side(n) | 1; }
// floats of one buffer (re and im plane); x at row stride n | 1 fits: n | 1 <= 2 ld
__host__ __device__ static inline long ctf_buf_floats(int n) { return 2L * n * ctf_ld(n); }
static inline size_t ctf_lds_bytes(int n) {
    return sizeof(float) * (2 * (size_t)n + (n <= CTF_ONDIE_MAX ? 2 * (size_t)ctf_buf_floats(n) : 0));
}

// H(ky, kx) from cf[5]; ky is the index in fftfreq order.  mode 1: the sign, -1 for H < 0 and +1 for anything else.
__device__ __forceinline__ float ctf_value(const double* __restrict__ cf, int ky, int kx, int n, int mode) {
    const int ks = ky < (n + 1) / 2 ? ky : ky - n;
    const double q = (double)(ks * ks + kx * kx) / (double)(n * n);
    double t = cf[2] * q + cf[3] * (q * q);
    t -= rint(t);
    double s, c;
    sincospi(2.0 * t, &s, &c);
    const float osc = (float)(cf[0] * s + cf[1] * c);
    const float h = osc * expf((float)(-cf[4] * q));
    if (mode == 1) return h < 0.f ? -1.f : 1.f;
    return h;
}

// grid = N * tiles (tile fastest), tiles = ceil(n R / 256).  H[N][n][R]
__global__ __launch_bounds__(CTF_THREADS) void ctf_eval_kernel(const double* __restrict__ coef, float* __restrict__ H, int n,
                                                               int tiles, int mode) {
    const int R = half_side(n);
    const unsigned row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const int e = (int)tile * CTF_THREADS + threadIdx.x;
    if (e >= n * R) return;
    const int ky = e / R, kx = e - ky * R;
    H[(size_t)row * n * R + e] = ctf_value(coef + 5 * (size_t)row, ky, kx, n, mode);
}

// stages 2 and 3: (Or + i Oi)(a, col) = sum_k (c + i SGN s)((a k) mod n) (Ir + i Ii)(k, col); a, k = 0 .. n - 1, col = 0 .. R - 1
template <int SGN>
__device__ __forceinline__ void ctf_columns(const float2* tw, const float* in, float* outp, int n, int R, int ld, int wave,
                                            int l31, int khalf) {
    const int TA = (n + 31) >> 5, TK = (R + 31) >> 5;
    const float* ir = in;
    const float* ii = in + (size_t)n * ld;
    float* orr = outp;
    float* oi = outp + (size_t)n * ld;
    for (int tile = wave; tile < TA * TK; tile += 4) {
        const int ta = tile / TK, tk = tile - ta * TK;
        const int a = ta * 32 + l31, col = tk * 32 + l31;
        const bool aok = a < n, cok = col < R;
        const int step = aok ? (2 * a) % n : 0;
        int t = aok ? (a * khalf) % n : 0;
        f32x16 accr, acci;
        zero(accr);
        zero(acci);
        for (int k0 = 0; k0 < n; k0 += 2) {
            const int k = k0 + khalf;
            const bool ok = cok && k < n;
            float br = 0.f, bi = 0.f;
            if (ok) {
                br = ir[(size_t)k * ld + col];
                bi = ii[(size_t)k * ld + col];
            }
            const float2 w = tw[t];
            const float wc = aok ? w.x : 0.f, wsn = aok ? (SGN > 0 ? w.y : -w.y) : 0.f;
            accr = __builtin_amdgcn_mfma_f32_32x32x2f32(wc, br, accr, 0, 0, 0);
            accr = __builtin_amdgcn_mfma_f32_32x32x2f32(-wsn, bi, accr, 0, 0, 0);
            acci = __builtin_amdgcn_mfma_f32_32x32x2f32(wc, bi, acci, 0, 0, 0);
            acci = __builtin_amdgcn_mfma_f32_32x32x2f32(wsn, br, acci, 0, 0, 0);
            tw_advance(t, step, n);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma_row(r, khalf, ta * 32);
            if (row < n && cok) {
                orr[(size_t)row * ld + col] = accr[r];
                oi[(size_t)row * ld + col] = acci[r];
            }
        }
    }
}

// grid = B.  X plane b at X + b x_stride, out[B][n][n] (may be X); exactly one of coef [B][5] and Hp (plane b at Hp + b h_stride)
template <bool ONDIE>
__global__ __launch_bounds__(CTF_THREADS) void ctf_filter_kernel(const float* X, long x_stride,
                                                                 const double* __restrict__ coef,
                                                                 const float* __restrict__ Hp, long h_stride, float* out,
                                                                 float* ws, int n, int mode) {
    extern __shared__ __attribute__((aligned(16))) float ctf_sm[];
    float2* const tw = reinterpret_cast<float2*>(ctf_sm);
    const int R = half_side(n), ld = ctf_ld(n), ldx = n | 1;
    const long buf = ctf_buf_floats(n);
    const size_t b = blockIdx.x;
    float* const buf0 = ONDIE ? ctf_sm + 2 * n : ws + b * 2 * buf;
    float* const buf1 = buf0 + buf;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int TI = (n + 31) >> 5, TK = (R + 31) >> 5;
    const size_t pl = (size_t)n * ld;                         // floats of a re or im plane

    dft_twiddles(tw, n, CTF_THREADS);
    {
        const float* x = X + b * x_stride;
        for (int e = tid; e < n * n; e += CTF_THREADS) {
            const int i = e / n, j = e - i * n;
            buf0[i * ldx + j] = x[e];
        }
    }
    __syncthreads();

    // ---- stage 1: rows.  A = x(i, j), B = (c, -s)((kx j) mod n) ----------------------------------------------------------------
    for (int tile = wave; tile < TI * TK; tile += 4) {
        const int ti = tile / TK, tk = tile - ti * TK;
        const int i = ti * 32 + l31, kx = tk * 32 + l31;
        const bool iok = i < n, kok = kx < R;
        const int step = kok ? (2 * kx) % n : 0;
        int t = kok ? (kx * khalf) % n : 0;
        f32x16 accr, acci;
        zero(accr);
        zero(acci);
        for (int j0 = 0; j0 < n; j0 += 2) {
            const int j = j0 + khalf;
            float a = 0.f;
            if (iok && j < n) a = buf0[i * ldx + j];
            const float2 w = tw[t];
            accr = __builtin_amdgcn_mfma_f32_32x32x2f32(a, kok ? w.x : 0.f, accr, 0, 0, 0);
            acci = __builtin_amdgcn_mfma_f32_32x32x2f32(a, kok ? -w.y : 0.f, acci, 0, 0, 0);
            tw_advance(t, step, n);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma_row(r, khalf, ti * 32);
            if (row < n && kok) {
                buf1[(size_t)row * ld + kx] = accr[r];
                buf1[pl + (size_t)row * ld + kx] = acci[r];
            }
        }
    }
    __syncthreads();

    // ---- stage 2: columns, G (buffer 1) -> F (buffer 0, x is no longer needed) -----------------------------------------------
    ctf_columns<-1>(tw, buf1, buf0, n, R, ld, wave, l31, khalf);
    __syncthreads();

    // ---- F *= H w: an element is read and written by one thread ----------------------------------------------------------------
    {
        const double* cf = coef ? coef + 5 * b : nullptr;
        const float* hp = Hp ? Hp + b * h_stride : nullptr;
        for (int e = tid; e < n * R; e += CTF_THREADS) {
            const int ky = e / R, kx = e - ky * R;
            float h;
            if (cf) {
                h = ctf_value(cf, ky, kx, n, mode);
            } else {
                h = hp[e];
                if (mode == 1) h = h < 0.f ? -1.f : 1.f;
            }
            h *= (kx == 0 || 2 * kx == n) ? 1.f : 2.f;        // exact
            const size_t at = (size_t)ky * ld + kx;
            buf0[at] *= h;
            buf0[pl + at] *= h;
        }
    }
    __syncthreads();

    // ---- stage 3: columns back, F (buffer 0) -> P (buffer 1) -------------------------------------------------------------------
    ctf_columns<1>(tw, buf0, buf1, n, R, ld, wave, l31, khalf);
    __syncthreads();

    // ---- stage 4: rows back.  A = (Pr, -Pi)(i, kx), B = (c, s)((kx j) mod n) -----------------------------------------------------
    const float scale = 1.f / ((float)n * (float)n);
    float* o = out + b * (size_t)n * n;
    for (int tile = wave; tile < TI * TI; tile += 4) {
        const int ti = tile / TI, tj = tile - ti * TI;
        const int i = ti * 32 + l31, j = tj * 32 + l31;
        const bool iok = i < n, jok = j < n;
        const int step = jok ? (2 * j) % n : 0;
        int t = jok ? (j * khalf) % n : 0;
        f32x16 acc;
        zero(acc);
        for (int k0 = 0; k0 < R; k0 += 2) {
            const int k = k0 + khalf;
            float ar = 0.f, ai = 0.f;
            if (iok && k < R) {
                ar = buf1[(size_t)i * ld + k];
                ai = buf1[pl + (size_t)i * ld + k];
            }
            const float2 w = tw[t];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, jok ? w.x : 0.f, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai, jok ? w.y : 0.f, acc, 0, 0, 0);
            tw_advance(t, step, n);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma_row(r, khalf, ti * 32);
            if (row < n && jok) o[(size_t)row * n + j] = scale * acc[r];
        }
    }
}

// grid = K * tiles (tile fastest), tiles = ceil(n R / 256).  D[K][n][R] (fp64), counts[K] (written by tile 0)
__global__ __launch_bounds__(CTF_THREADS) void ctf_power_kernel(const double* __restrict__ coef,
                                                                const int* __restrict__ order, const int* __restrict__ seg,
                                                                double* __restrict__ D, int* __restrict__ counts, int N,
                                                                int n, int tiles) {
    __shared__ int red[CTF_THREADS];
    const int R = half_side(n);
    const int k = blockIdx.x / tiles, tile = blockIdx.x - k * tiles;
    // cleaned boundaries of class k: min(max(0, seg[0], ..., seg[k]), N) and the same with seg[k + 1]
    int m = 0;
    for (int q = threadIdx.x; q <= k; q += CTF_THREADS) m = max(m, seg[q]);
    red[threadIdx.x] = m;
    __syncthreads();
#pragma unroll
    for (int s = CTF_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const int run = red[0];
    const int sk = min(run, N), ek = min(max(run, seg[k + 1]), N);
    if (tile == 0 && threadIdx.x == 0) {
        int c = 0;
        for (int p = sk; p < ek; ++p) {
            const int id = order[p];
            c += id >= 0 && id < N;
        }
        counts[k] = c;
    }
    const int e = tile * CTF_THREADS + threadIdx.x;
    if (e >= n * R) return;
    const int ky = e / R, kx = e - ky * R;
    double sum = 0.0;
    for (int p = sk; p < ek; ++p) {
        const int id = order[p];
        if (id < 0 || id >= N) continue;
        const double h = (double)ctf_value(coef + 5 * (size_t)id, ky, kx, n, 0);
        sum += h * h;
    }
    D[(size_t)k * n * R + e] = sum;
}

}  // namespace tvae_cluster
