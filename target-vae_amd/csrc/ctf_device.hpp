// The stages of the on-die direct DFT that ctf_filter_kernel (ctf_kernels.hpp) and the kernels of spectrum_kernels.hpp share:
// geometry of the two buffers, the load of a plane, rows forward, columns either way, the multiply with a real H and rows
// back.  Device and host helpers only, NO __global__ function (cluster_common.hpp says why), so any unit may include it.
// Every function is called by all 256 threads of the workgroup and contains no barrier: the caller places one between stages.
// ctf_kernels.hpp describes the layout (buffer 0: x at row stride n | 1, then F; buffer 1: G, then P; re plane, im plane at row
// stride ld) and the arithmetic: fp32 FMA chains on v_mfma_f32_32x32x2_f32 in ascending k, twiddles from the integer-reduced
// table, predicated zeros outside the plane.
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

// H(ky, kx) from cf[5] (ctf_kernels.hpp states the arithmetic); ky is the index in fftfreq order.  mode 1: the sign, -1 for H < 0 and +1 for anything else.
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

// the lane's place in its wave and the wave's in the workgroup
struct CtfLane {
    int tid, wave, l31, khalf;
};
__device__ __forceinline__ CtfLane ctf_lane() {
    CtfLane L;
    L.tid = threadIdx.x;
    const int lane = L.tid & 63;
    L.wave = __builtin_amdgcn_readfirstlane(L.tid >> 6);
    L.l31 = lane & 31;
    L.khalf = lane >> 5;
    return L;
}

// x[n][n] -> buffer 0 at row stride ldx = n | 1
__device__ __forceinline__ void ctf_load_plane(const float* x, float* buf0, int n, int tid) {
    const int ldx = n | 1;
    for (int e = tid; e < n * n; e += CTF_THREADS) {
        const int i = e / n, j = e - i * n;
        buf0[i * ldx + j] = x[e];
    }
}

// stage 1: rows.  A = x(i, j) (buffer 0, row stride n | 1), B = (c, -s)((kx j) mod n); G(i, kx) -> buffer 1
__device__ __forceinline__ void ctf_rows(const float2* tw, const float* buf0, float* buf1, int n, int R, int ld, int wave,
                                         int l31, int khalf) {
    const int ldx = n | 1;
    const int TI = (n + 31) >> 5, TK = (R + 31) >> 5;
    const size_t pl = (size_t)n * ld;
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

// F *= H w_kx: h(ky, kx, e = ky R + kx) is the caller's source of H; the Hermitian weight is exact, so H w is one rounding.
// An element is read and written by one thread.
template <class HFn>
__device__ __forceinline__ void ctf_multiply(float* buf0, int n, int R, int ld, int tid, HFn h_of) {
    const size_t pl = (size_t)n * ld;
    for (int e = tid; e < n * R; e += CTF_THREADS) {
        const int ky = e / R, kx = e - ky * R;
        float h = h_of(ky, kx, e);
        h *= (kx == 0 || 2 * kx == n) ? 1.f : 2.f;            // exact
        const size_t at = (size_t)ky * ld + kx;
        buf0[at] *= h;
        buf0[pl + at] *= h;
    }
}

// stage 4: rows back.  A = (Pr, -Pi)(i, kx) (buffer 1), B = (c, s)((kx j) mod n); o[n][n] = n^-2 Re(...)
__device__ __forceinline__ void ctf_rows_back(const float2* tw, const float* buf1, float* o, int n, int R, int ld, int wave,
                                              int l31, int khalf) {
    const int TI = (n + 31) >> 5;
    const size_t pl = (size_t)n * ld;
    const float scale = 1.f / ((float)n * (float)n);
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

}  // namespace tvae_cluster
