// Device helpers shared by the kernel families: wave / workgroup reductions, the activations, the first decoder layer's
// pre-activation.  No __global__ function, so any family may include it (the kernels: small_kernels.hpp, abi_small.hip alone).
#pragma once
#include "gemm_f32_mfma.hpp"

namespace tvae {

constexpr float EPS_STD = 1e-6f;      // reference train_mnist.py:197

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
    return v;
}

template <int CTRL>
__device__ __forceinline__ float dpp_get(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
// Sums EIGHT values over the 64 lanes of a wave in 4 + 2 + 1 + 3 exchange steps (a butterfly that halves the number of
// live values at each of the first three steps) instead of 8 x 6: lane l returns the total of value (l & 7).
__device__ __forceinline__ float wave_sum8(const float (&a)[8], int lane) {
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
    float b[4], c[2];
#pragma unroll
    for (int i = 0; i < 4; ++i)      // lane keeps index 2i + b0, its partner (lane ^ 1) sends exactly that one
        b[i] = (b0 ? a[2 * i + 1] : a[2 * i]) + dpp_get<0xB1>(b0 ? a[2 * i] : a[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 2; ++i)      // b index 2i + b1 -> original index 4i + 2 b1 + b0
        c[i] = (b1 ? b[2 * i + 1] : b[2 * i]) + dpp_get<0x4E>(b1 ? b[2 * i] : b[2 * i + 1]);
    float d = (b2 ? c[1] : c[0]) + __shfl_xor(b2 ? c[0] : c[1], 4, 64);     // original index 4 b2 + 2 b1 + b0 = lane & 7
    d += __shfl_xor(d, 8, 64);
    d += __shfl_xor(d, 16, 64);
    d += __shfl_xor(d, 32, 64);
    return d;
}

// the same for FOUR values (2 + 1 + 4 exchange steps): lane l returns the total of value (l & 3)
__device__ __forceinline__ float wave_sum4(const float (&a)[4], int lane) {
    const bool b0 = lane & 1, b1 = lane & 2;
    float b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) b[i] = (b0 ? a[2 * i + 1] : a[2 * i]) + dpp_get<0xB1>(b0 ? a[2 * i] : a[2 * i + 1]);
    float d = (b1 ? b[1] : b[0]) + dpp_get<0x4E>(b1 ? b[0] : b[1]);          // original index 2 b1 + b0 = lane & 3
    d += __shfl_xor(d, 4, 64);
    d += __shfl_xor(d, 8, 64);
    d += __shfl_xor(d, 16, 64);
    d += __shfl_xor(d, 32, 64);
    return d;
}

// Sum NV values over the workgroup; every thread returns with the totals.  sm: >= NV*16 floats.
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float s = wave_sum(v[i]);
        if (lane == 0) sm[i * 16 + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += sm[i * 16 + w];
        v[i] = s;
    }
}
__device__ __forceinline__ float block_max(float v, float* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    const float s = wave_max(v);
    if (lane == 0) sm[wave] = s;
    __syncthreads();
    float m = sm[0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, sm[w]);
    return m;
}

__device__ __forceinline__ float act_apply(float x, int act, float slope) {
    if (act == ACT_LRELU) return x > 0.f ? x : x * slope;
    if (act == ACT_TANH) return tanhf(x);
    return x;
}
__device__ __forceinline__ float act_deriv_from_out(float y, int act, float slope) {
    if (act == ACT_LRELU) return y > 0.f ? 1.f : slope;
    if (act == ACT_TANH) return 1.f - y * y;
    return 1.f;
}

// pre-activation of the first decoder layer, with a FIXED operation order: the kernels that recompute this layer
// instead of reading its stored output (dense_x6_kernels.hpp, VirtAct) must reproduce it bit for bit so that the
// activation masks of forward and backward agree
__device__ __forceinline__ float dec_l0_pre(float w0, float w1, float bc, float lb, float x0, float x1) {
    return __fmaf_rn(w1, x1, __fmaf_rn(w0, x0, bc)) + lb;
}

}  // namespace tvae
