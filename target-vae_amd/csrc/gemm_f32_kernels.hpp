// The non-template kernels of the fp32 MFMA GEMM family (gemm_f32_mfma.hpp).  Included by abi_linear_f32.hip ALONE (every unit
// that sees a non-template kernel emits it); the other units reach splitk_finalize_kernel through abi_common.hpp: splitk_finalize.
#pragma once
#include "gemm_f32_mfma.hpp"

namespace tvae {

// Both operands by LDS-DMA: A(row x, red k) at At[k*lda + x] (x contiguous: W^T for forward, W itself for dgrad),
// B(k, n) at X[k*ldx + n].  No register staging at all: per k-step a wave issues 4 DMA instructions, reads 32
// fragments and issues 32 MFMAs.  Both LDS tiles are unpadded [BK][128].
static __global__ __launch_bounds__(GEMM_THREADS, 4)
void gemm_f32_glds2_kernel(const float* __restrict__ At, long lda, const float* __restrict__ X, long ldx, Epilogue ep,
                           int M, int N, int K, TileMap tm, int vec_ep) {
    constexpr int TT = BK * BN;                      // one operand tile (floats)
    __shared__ __attribute__((aligned(16))) float lds[4 * TT > 64 * EP_LD ? 4 * TT : 64 * EP_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    int tile_m, tile_n, split_unused;
    if (!tm.decode(blockIdx.x, tile_m, tile_n, split_unused)) return;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int nk = K / BK;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const float* asrc[2];
    const float* bsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = i * 4 + wave;                  // chunk c = k rows 2c, 2c+1 of a tile
        asrc[i] = At + (long)(2 * c + (lane >> 5)) * lda + m0 + (lane & 31) * 4;
        bsrc[i] = X + (long)(2 * c + (lane >> 5)) * ldx + n0 + (lane & 31) * 4;
    }
    auto dma = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = i * 4 + wave;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)asrc[i],
                                             (__attribute__((address_space(3))) void*)(buf + c * 256), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)bsrc[i],
                                             (__attribute__((address_space(3))) void*)(buf + TT + c * 256), 16, 0, 0);
            asrc[i] += (long)BK * lda;
            bsrc[i] += (long)BK * ldx;
        }
    };
    if (nk > 0) dma(lds);
    __syncthreads();
    const int arow = wm * 64 + (lane & 31);
    const int bcol = wn * 64 + (lane & 31);
    const int khalf = lane >> 5;
    for (int t = 0; t < nk; ++t) {
        const int cur = t & 1;
        if (t + 1 < nk) dma(lds + (cur ^ 1) * (2 * TT));
        const float* as = lds + cur * (2 * TT);
        const float* bs = as + TT;
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const int kk = 2 * s + khalf;
            const float a0 = as[kk * BN + arow];
            const float a1 = as[kk * BN + arow + 32];
            const float b0 = bs[kk * BN + bcol];
            const float b1 = bs[kk * BN + bcol + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    if (vec_ep) tile_epilogue_v4(acc, lds, ep, m0, n0);
    else tile_epilogue(acc, lds, ep, m0, M, n0 + (tid & 127), (n0 + (tid & 127)) < N, nullptr, 0, N);
}

// out[c][r] = in[r][c]   (small weight transposes feeding the DMA forward GEMM)
static __global__ void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols) {
    __shared__ float t[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int r = by + j, c = bx + threadIdx.x;
        if (r < rows && c < cols) t[j][threadIdx.x] = in[(long)r * cols + c];
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int c = bx + j, r = by + threadIdx.x;
        if (r < rows && c < cols) out[(long)c * rows + r] = t[threadIdx.x][j];
    }
}

// Deterministic reduction of the split-K slabs: a workgroup owns 64 consecutive outputs, its four thread rows sum
// every fourth slab (independent loads in flight, 256-byte coalesced rows) and the four partial sums are added in a
// fixed order.  (A thread per output walking all slabs is latency bound when there are hundreds of small slabs.)
static __global__ __launch_bounds__(256) void splitk_finalize_kernel(const float* ws, int splits, int M, int N, Epilogue ep) {
    __shared__ float part[4][64];
    const long total = (long)M * N;
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    for (long base = (long)blockIdx.x * 64; base < total; base += (long)gridDim.x * 64) {
        const long i = base + lane;
        float s = 0.f;
        if (i < total) {
            int k = slice;
            for (; k + 12 < splits; k += 16) {
                const float a = ws[(long)k * total + i], b = ws[(long)(k + 4) * total + i];
                const float c = ws[(long)(k + 8) * total + i], d = ws[(long)(k + 12) * total + i];
                s += (a + b) + (c + d);
            }
            for (; k < splits; k += 4) s += ws[(long)k * total + i];
        }
        part[slice][lane] = s;
        __syncthreads();
        if (slice == 0 && i < total) {
            const float v = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
            const int m = (int)(i / N), n = (int)(i - (long)m * N);
            ep.store(m, n, ep.prep(n), v);
        }
        __syncthreads();
    }
}

}  // namespace tvae
