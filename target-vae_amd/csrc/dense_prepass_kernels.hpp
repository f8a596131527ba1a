// Pre-passes of the split-pipe dense layers (dense_x6_kernels.hpp): the weight split into fragment-ready cells, row maxima and
// sums, the operand bounds of h3.  Non-template kernels: included by abi_dense_x6.hip ALONE, others call its launchers (abi_dense_x6.hpp).
#pragma once
#include "conv_x6_device.hpp"

namespace tvae {

// Pre-pass: W fp32 -> cells [part][octet][row < Rpad].
//   transpose == 0: A(row, k) = W[row*ldw + k]        (forward: rows = out features, k = in features)
//   transpose == 1: A(row, k) = W[k*ldw + row]        (data gradient: rows = in features, k = out features)
// Rows >= Rrows and k >= K are zero; K8pad octets (even).  scale (optional, [K]): A(row, k) is multiplied by scale[k]
// before the split (one fp32 rounding, as an elementwise fp32 product would have).
static __global__ void dense_split3_kernel(const float* __restrict__ W, long ldw, uint4* __restrict__ A3, int Rrows, int Rpad,
                                           int K, int K8pad, int transpose, const float* __restrict__ scale) {
    const long total = (long)K8pad * Rpad;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int row = (int)(i % Rpad);
        const int o = (int)(i / Rpad);
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * o + j;
            r[j] = (row < Rrows && k < K) ? (transpose ? W[(long)k * ldw + row] : W[(long)row * ldw + k]) : 0.f;
            if (scale && k < K) r[j] *= scale[k];
        }
        Cell16 h, m, l;
        split3x8(r, h, m, l);
        A3[i] = h.u;
        A3[total + i] = m.u;
        A3[2 * total + i] = l.u;
    }
}

// The same pre-pass in the h3 arithmetic: cells [part < 2][octet][row] of fp16 parts of A(row, k) * s[row],
// s[row] = h3_scale(rowmax[row]), rowmax[row] = max_k |A(row, k)| (dense_rowmax_kernel): ONE POWER OF TWO PER ROW (round 4).
// A row of the operand is a row of the product, so the scale is undone per accumulator row in the GEMM's epilogue and a
// row that lies 2^20 below the rest of the matrix (a dead unit, a filter that has not started to train) is computed with
// the same relative accuracy as any other.  The row maxima live in the first Rpad words behind the two parts
// (A3[2 * total]: the buffer is sized for three parts), where the GEMM finds them again.
// Block = 64 rows x 16 k-slices, like dense_rowsum_kernel; rows >= Rrows (padding) get 0.
static __global__ __launch_bounds__(1024) void dense_rowmax_kernel(const float* __restrict__ W, long ldw, int Rrows, int Rpad,
                                                                   int K, int transpose, const float* __restrict__ scale,
                                                                   float* __restrict__ rowmax) {
    __shared__ float part[16][64];
    const int r = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int row = blockIdx.x * 64 + r;
    float mx = 0.f;
    if (row < Rrows)
        for (int k = sl; k < K; k += 16) {
            float v = transpose ? W[(long)k * ldw + row] : W[(long)row * ldw + k];
            if (scale) v *= scale[k];
            mx = fmaxf(mx, fabsf(v));
        }
    part[sl][r] = mx;
    __syncthreads();
    if (sl == 0 && row < Rpad) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) t = fmaxf(t, part[q][r]);
        rowmax[row] = t;
    }
}
// The same for a row-major operand (transpose == 0), where the kernel above has every lane on a row of its own (64 rows x 4 B
// per load instruction): one WAVE per row, lanes along k (19 -> ~6 us for a 512 x 512 weight).  Block = 4 rows.
static __global__ __launch_bounds__(256) void dense_rowmax_rows_kernel(const float* __restrict__ W, long ldw, int Rrows, int Rpad,
                                                                      int K, const float* __restrict__ scale,
                                                                      float* __restrict__ rowmax) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Rpad) return;
    float mx = 0.f;
    if (row < Rrows)
        for (int k = lane; k < K; k += 64) {
            float v = W[(long)row * ldw + k];
            if (scale) v *= scale[k];
            mx = fmaxf(mx, fabsf(v));
        }
    mx = h3_wave_max(mx);
    if (lane == 0) rowmax[row] = mx;
}
static __global__ void h3_zero_slots_kernel(float* p, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0.f;
}
// rowmax: one maximum per row of the operand (row = i % Rpad, the stacked row index of batched operands)
static __global__ void dense_split2h_kernel(const float* __restrict__ W, long ldw, uint4* __restrict__ A3, int Rrows, int Rpad,
                                            int K, int K8pad, int transpose, const float* __restrict__ scale,
                                            const float* __restrict__ rowmax) {
    const long total = (long)K8pad * Rpad;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        // row-major operands (forward form): consecutive threads take consecutive octets of a ROW, i.e. consecutive 32-byte
        // pieces of memory -- with the row fastest every lane of a load touched its own 768-byte-strided line (the spectral
        // weight's 77 MB: 100 -> 60 us); the 16-byte cell stores of eight neighbouring rows still complete one line.
        // Transposed operands keep the row fastest (there it IS the contiguous index).
        const int row = transpose ? (int)(i % Rpad) : (int)(i / K8pad);
        const int o = transpose ? (int)(i / Rpad) : (int)(i % K8pad);
        const long ci = (long)o * Rpad + row;            // cell index
        const float s = h3_scale(rowmax[row]);
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * o + j;
            r[j] = (row < Rrows && k < K) ? (transpose ? W[(long)k * ldw + row] : W[(long)row * ldw + k]) : 0.f;
            if (scale && k < K) r[j] *= scale[k];
            r[j] *= s;
        }
        Cell16 h, l;
        split2hx8(r, h, l);
        A3[ci] = h.u;
        A3[total + ci] = l.u;
    }
}

// The same split for row-major operands (transpose == 0) with BOTH sides coalesced: a workgroup takes 32 rows; its threads read
// consecutive octets of a row (consecutive 32-byte pieces of memory), park the cells in LDS as [octet][row] and write each
// octet's 32 cells as one 512-byte run (the kernel above stores 16-byte cells 16 Rpad bytes apart: 62 us for the 38 MB of the
// spectral weight; this one ~25).  Dynamic LDS: 32 K8pad cells x 2 parts.
static __global__ __launch_bounds__(256) void dense_split2h_rows_kernel(const float* __restrict__ W, long ldw, uint4* __restrict__ A3,
                                                                        int Rrows, int Rpad, int K, int K8pad,
                                                                        const float* __restrict__ scale,
                                                                        const float* __restrict__ rowmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char split_lds[];
    uint4* Hs = reinterpret_cast<uint4*>(split_lds);
    uint4* Ls = Hs + 32 * K8pad;
    const long total = (long)K8pad * Rpad;
    const int r0 = blockIdx.x * 32, ncell = 32 * K8pad;
    const bool vec = (ldw & 3) == 0 && (reinterpret_cast<size_t>(W) & 15) == 0;
    for (int c = threadIdx.x; c < ncell; c += 256) {
        const int rl = c / K8pad, o = c - rl * K8pad, row = r0 + rl;
        const float s = h3_scale(rowmax[row]);
        float r[8];
        if (vec && row < Rrows && 8 * o + 8 <= K) {      // two 16-byte loads
            const float4 a = *reinterpret_cast<const float4*>(W + (long)row * ldw + 8 * o);
            const float4 b = *reinterpret_cast<const float4*>(W + (long)row * ldw + 8 * o + 4);
            r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 8 * o + j;
                r[j] = (row < Rrows && k < K) ? W[(long)row * ldw + k] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * o + j;
            if (scale && k < K) r[j] *= scale[k];
            r[j] *= s;
        }
        Cell16 h, l;
        split2hx8(r, h, l);
        Hs[o * 32 + rl] = h.u;
        Ls[o * 32 + rl] = l.u;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < ncell; c += 256) {
        const int o = c >> 5, rl = c & 31;
        const long ci = (long)o * Rpad + r0 + rl;
        A3[ci] = Hs[c];
        A3[total + ci] = Ls[c];
    }
}

// h3 scale of the recomputed first-layer activation (VirtAct): slots[0] = max |xr|, slots[1] = max_k (|wc[k][0]| + |wc[k][1]|),
// slots[2] = max_{b,k} |bc[k] + lb[b][k]| (atomic maxima into zeroed slots); |act(pre)| <= |pre| <= slots[1] slots[0] + slots[2]
// for LeakyReLU (slope <= 1), tanh and the identity.  slots[3] is the caller's (max |gy| of the weight gradient) and
// slots[4 + k] = max_b |bc[k] + lb[b][k]|: with it a consumer whose operand ROW is feature k (the weight gradient) bounds that
// row alone, (|wc[k][0]| + |wc[k][1]|) slots[0] + slots[4 + k].
static __global__ void dec_l0_bound_kernel(const float* __restrict__ xr, long nxr, const float* __restrict__ wc,
                                           const float* __restrict__ bc, const float* __restrict__ lb, long nlb, int K,
                                           float* __restrict__ slots) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x, gsz = (long)gridDim.x * blockDim.x;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    const long n4 = (reinterpret_cast<size_t>(xr) & 15) == 0 ? nxr / 4 : 0;        // 16-byte loads, several in flight
    const float4* x4 = reinterpret_cast<const float4*>(xr);
#pragma unroll 4
    for (long i = gid; i < n4; i += gsz) {
        const float4 v = x4[i];
        m0 = fmaxf(fmaxf(m0, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    for (long i = 4 * n4 + gid; i < nxr; i += gsz) m0 = fmaxf(m0, fabsf(xr[i]));
    for (long i = gid; i < K; i += gsz) m1 = fmaxf(m1, fabsf(wc[2 * i]) + fabsf(wc[2 * i + 1]));
    if (lb) {
        // thread = (feature k, one of 16 image chunks): a local maximum over its images, then ONE atomic per thread (one atomic
        // per (image, feature) pair -- 256 per word at the bench shape -- made this loop the kernel's cost)
        const long nimg = nlb / K, per = (nimg + 15) / 16;
        for (long t = gid; t < 16L * K; t += gsz) {
            const int k = (int)(t % K);
            const long b0 = (t / K) * per, b1 = b0 + per < nimg ? b0 + per : nimg;
            float v = 0.f;
            for (long b = b0; b < b1; ++b) v = fmaxf(v, fabsf(bc[k] + lb[b * K + k]));
            if (b1 > b0) {
                m2 = fmaxf(m2, v);
                h3_atomic_amax(slots + 4 + k, v);
            }
        }
    } else {
        for (long i = gid; i < K; i += gsz) {
            m2 = fmaxf(m2, fabsf(bc[i]));
            slots[4 + i] = fabsf(bc[i]);
        }
    }
    h3_block_amax(m0, slots);
    h3_block_amax(m1, slots + 1);
    h3_block_amax(m2, slots + 2);
}

// rowsum[row] = sum_k A(row, k) of the (scaled) operand above (VirtGrad.csum).  Block = 64 rows x 16 k-slices; the slice
// sums are added in slice order (deterministic).
static __global__ __launch_bounds__(1024) void dense_rowsum_kernel(const float* __restrict__ W, long ldw, int Rrows, int K,
                                                                   int transpose, const float* __restrict__ scale,
                                                                   float* __restrict__ rowsum) {
    __shared__ float part[16][64];
    const int r = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int row = blockIdx.x * 64 + r;
    float s = 0.f;
    if (row < Rrows)
        for (int k = sl; k < K; k += 16) {
            float v = transpose ? W[(long)k * ldw + row] : W[(long)row * ldw + k];
            if (scale) v *= scale[k];
            s += v;
        }
    part[sl][r] = s;
    __syncthreads();
    if (sl == 0 && row < Rrows) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += part[q][r];
        rowsum[row] = t;
    }
}
}  // namespace tvae
