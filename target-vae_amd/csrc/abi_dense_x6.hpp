// Host-side declarations shared by the split-pipe dense units (abi_dense_x6.hip, abi_dense_wgrad_x6.hip) and the
// frequency-domain convolution (abi_conv_dft.hip), which runs its spectral contraction as batched launches of them.
#pragma once
#include "abi_common.hpp"
#include "dense_x6_kernels.hpp"

namespace tvae {

// k-octets of the weight cells: whole 16-k steps
static inline int dense_k8pad(int K) { return x6_round_up((K + 7) / 8, 2); }
static inline long dense_x6_bytes(int rows, int K) {
    const long Rpad = x6_round_up(rows, DX6_ROWS), K8pad = dense_k8pad(K);
    return 3 * K8pad * Rpad * 16;
}

// shapes of the spectral contraction with the streamed panel resident in LDS (dense_x6_batched_xres): 8, 10 or 12 k-steps, two
// or three parts, whole 128-column panels, whole 512-row problems, its LDS within a CU.  Host arithmetic only: the route query of
// the frequency-domain convolution (tvae_conv1_dft_route) asks it on machines without a device.
static inline bool dense_x6_xres_fits(int rows_per_problem, int Mb, int N, int K, int parts) {
    const int nk = dense_k8pad(K) / 2;
    const size_t lds = (size_t)nk * parts * 256 * 16 + (size_t)(Mb + 128) * 4;
    return (parts == 2 || parts == 3) && (nk == 12 || nk == 10 || nk == 8) && N % 128 == 0 && rows_per_problem % DX6_ROWS == 0 &&
           Mb >= rows_per_problem && lds <= X6_LDS_MAX;
}

// h3 cells (tvae_dense_split2h): one maximum per padded row (and, behind them, scratch words of the GEMM entry points) behind
// the two part arrays
static inline float* h3_trailer(const void* a3, int rows, int K) {
    const long total = (long)dense_k8pad(K) * x6_round_up(rows, DX6_ROWS);
    return reinterpret_cast<float*>(const_cast<void*>(a3)) + 2 * total * 4;
}

// raw launcher of dense_x6_kernel<XV, NP, EPI>: declared here, defined and instantiated once per entry of
// dense_x6_instances.def, each in an object of its own (dense_x6_instance.hip); abi_dense_x6.hip looks them up by (xv, epi, parts)
#define TVAE_DX6_LAUNCH_ARGS                                                                                          \
    const uint4 *a3, const float *X, long ldx, const Epilogue &ep, int M, int Mpad, int N, int K, int K8pad,          \
        const TileMap &tm, const DenseBatch &bt, const ColDot &cd, const InTail &it, const VirtGrad &vg,              \
        const VirtAct &va, hipStream_t st, const H3Scale &hs
template <int XV, int EPI, int NP>
TVAE_INTERNAL int dense_x6_launch(TVAE_DX6_LAUNCH_ARGS);

// weight-gradient launchers, one object per number of parts (dense_wgrad_x6_instance.hip)
#define TVAE_WG_LAUNCH_ARGS                                                                                           \
    int variant, const float *dY, long ldd, const float *X, long ldx, float *ws, int M, int Kf, int N, int nchunk,     \
        const TileMap &tm, const DenseBatch &bt, long dy_stride, const VirtGrad &vg, const VirtAct &va,               \
        const ATile &atile, hipStream_t st, const H3Scale &hs
TVAE_INTERNAL int dense_wgrad_x6_launch_p3(TVAE_WG_LAUNCH_ARGS);
TVAE_INTERNAL int dense_wgrad_x6_launch_p2(TVAE_WG_LAUNCH_ARGS);
TVAE_INTERNAL int dense_wgrad_x6_launch_p1(TVAE_WG_LAUNCH_ARGS);
// one-part mode with the A operand STORED as bf16 (dense_wgrad_x6_dma_kernel<.., ABF>)
TVAE_INTERNAL int dense_wgrad_x6_launch_p1_abf(TVAE_WG_LAUNCH_ARGS);

// the exact-fit 256 x 192 tile of the spectral weight gradient (dense_wgrad_x6_wide_kernel; tm / bt count 256-row tiles)
#define TVAE_WGW_LAUNCH_ARGS                                                                                          \
    const float *dY, long ldd, const float *X, long ldx, float *ws, int M, int Kf, int N, int nchunk, const TileMap &tm, \
        const DenseBatch &bt, long dy_stride, const ATile &atile, hipStream_t st, const H3Scale &hs
TVAE_INTERNAL int dense_wgrad_x6_wide_p3(TVAE_WGW_LAUNCH_ARGS);
TVAE_INTERNAL int dense_wgrad_x6_wide_p2(TVAE_WGW_LAUNCH_ARGS);

// pre-pass kernels that other units launch as well (dense_prepass_kernels.hpp, compiled in abi_dense_x6.hip alone): each launches
// and returns the error of the launch
TVAE_INTERNAL int h3_zero_slots(float* p, int n, int threads, hipStream_t st);
// (dense_split2h_rows_kernel for row-major operands of <= 48 k-octets: both sides coalesced through <= 48 KB of LDS)
TVAE_INTERNAL int dense_split2h(const float* W, long ldw, uint4* a3, int rows, int Rpad, int K, int K8pad, int transpose,
                                const float* scale, const float* rowmax, hipStream_t st);
// N columns (pixels) of xr [N][2]; nlb floats of lb (0: none)
TVAE_INTERNAL int dec_l0_bound(const float* xr, int N, const float* wc, const float* bc, const float* lb, long nlb, int K,
                               float* slots, hipStream_t st);

// the same with the 256-row / four-wave tile (dense_x6_plain4_kernel: short reductions); tm / bt count 256-row tiles
TVAE_INTERNAL int dense_x6_batched4(const void* w3, const float* X, long ldx, const Epilogue& ep, int rows_per_problem,
                                    int rows_total, int N, int K, const TileMap& tm, const DenseBatch& bt, int parts,
                                    hipStream_t st, H3Scale hs = H3_NONE, bool out_bf16 = false);
// the spectral contraction with the streamed panel resident in LDS (dense_x6_xres_kernel); false: shape not handled, nothing launched
TVAE_INTERNAL bool dense_x6_batched_xres(const void* w3, const float* X, long ldx, const Epilogue& ep, int rows_per_problem,
                                         int Mb, int nprob, int N, int K, long x_stride, long c_stride, int parts,
                                         hipStream_t st, H3Scale hs, int* rc);
// batched forward GEMM of the spectral contraction: rows of all problems stacked in w3 (abi_dense_x6.hip)
TVAE_INTERNAL int dense_x6_batched(const void* w3, const float* X, long ldx, const Epilogue& ep, int rows_per_problem,
                                   int rows_total, int N, int K, const TileMap& tm, const DenseBatch& bt, int parts,
                                   hipStream_t st, H3Scale hs = H3_NONE);
// batched weight-gradient GEMM into split-K slabs (abi_dense_wgrad_x6.hip)
TVAE_INTERNAL int dense_wgrad_x6_batched(const float* dY, long ldd, const float* X, long ldx, float* slabs, int M,
                                         int Kf, int N, int nchunk, const TileMap& tm, const DenseBatch& bt,
                                         long dy_stride, const ATile& atile, int parts, hipStream_t st,
                                         H3Scale hs = H3_NONE, bool a_bf16 = false, bool wide = false);

}  // namespace tvae
