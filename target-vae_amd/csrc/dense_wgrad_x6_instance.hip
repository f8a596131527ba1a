// libtvae_hip.so: the weight-gradient kernels of the split-pipe dense layers (dense_x6_kernels.hpp: dense_wgrad_x6_dma_kernel,
// dense_wgrad_x6_wide_kernel) for ONE number of parts, chosen on the command line (-DTVAE_WG_NP=1 | 2 | 3, set by the Makefile's
// pattern rule from the object's name), and their launchers.  1: one-part bf16 throughput mode, 2: h3 arithmetic (two fp16
// parts, three products), 3: exact three-part split.
#include "abi_dense_x6.hpp"

using namespace tvae;

// variant = VIRT | XVA << 1 | LRF << 2   (LRF: 0 off, 1 two-valued from H, 2 two-valued from sign bits)
// Variant 11 (sign bits against gy x the recomputed first-layer operand) runs in 32-column steps (STEP = 32, a ring of its own
// size) when the reduction slices and the images are multiples of 32 columns; -DTVAE_WG_STEP16 keeps the 16-column instance
// everywhere (the A/B partner: profiles/tools/build_variant.sh dense_wgrad_x6_p2 -DTVAE_WG_STEP16 old.so).
#ifdef TVAE_WG_STEP16
constexpr bool WG_STEP32 = false;
#else
constexpr bool WG_STEP32 = true;
#endif
#define TVAE_WG_BITS_XVA(NP_)                                                                                         \
    do {                                                                                                              \
        if constexpr (WG_STEP32) {                                                                                    \
            if (nchunk % 32 == 0 && N % 32 == 0 && va.Np >= 32 && va.Np % 32 == 0) {                                  \
                hipError_t e_ = allow_big_lds(dense_wgrad_x6_dma_kernel<true, true, 2, NP_, false, 32>, WG32_RING_BYTES); \
                if (e_ != hipSuccess) return (int)e_;                                                                 \
                hipLaunchKernelGGL((dense_wgrad_x6_dma_kernel<true, true, 2, NP_, false, 32>), dim3(tm.grid()),       \
                                   dim3(DX6_THREADS), WG32_RING_BYTES, st, dY, ldd, X, ldx, ws, M, Kf, N, nchunk, tm, bt, \
                                   dy_stride, vg, va, atile, hs);                                                     \
                return (int)hipGetLastError();                                                                        \
            }                                                                                                         \
        }                                                                                                             \
        TVAE_WG_ONE(true, true, 2, NP_);                                                                              \
    } while (0)
#define TVAE_WG_ONE(V_, X_, L_, NP_)                                                                                  \
    do {                                                                                                              \
        hipError_t e_ = allow_big_lds(dense_wgrad_x6_dma_kernel<V_, X_, L_, NP_>, WG_RING_BYTES);                     \
        if (e_ != hipSuccess) return (int)e_;                                                                         \
        hipLaunchKernelGGL((dense_wgrad_x6_dma_kernel<V_, X_, L_, NP_>), dim3(tm.grid()), dim3(DX6_THREADS),           \
                           WG_RING_BYTES, st, dY, ldd, X, ldx, ws, M, Kf, N, nchunk, tm, bt, dy_stride, vg, va, atile, hs); \
        return (int)hipGetLastError();                                                                                \
    } while (0)
#define TVAE_WG_LAUNCH_DEF(NP_)                                                                                       \
    namespace tvae {                                                                                                  \
    int dense_wgrad_x6_launch_p##NP_(TVAE_WG_LAUNCH_ARGS) {                                                           \
        switch (variant) {                                                                                            \
            case 0: TVAE_WG_ONE(false, false, 0, NP_);                                                            \
            case 1: TVAE_WG_ONE(true, false, 0, NP_);                                                             \
            case 2: TVAE_WG_ONE(false, true, 0, NP_);                                                             \
            case 3: TVAE_WG_ONE(true, true, 0, NP_);                                                              \
            case 5: TVAE_WG_ONE(true, false, 1, NP_);                                                                 \
            case 7: TVAE_WG_ONE(true, true, 1, NP_);                                                                  \
            case 9: TVAE_WG_ONE(true, false, 2, NP_);                                                                 \
            case 11: TVAE_WG_BITS_XVA(NP_);                                                                           \
            default: return (int)hipErrorInvalidValue;                                                                \
        }                                                                                                             \
    }                                                                                                                 \
    }

#define TVAE_WG_LAUNCH_DEF_ABF                                                                                        \
    namespace tvae {                                                                                                  \
    int dense_wgrad_x6_launch_p1_abf(TVAE_WG_LAUNCH_ARGS) {                                                           \
        if (variant != 0) return (int)hipErrorInvalidValue;                                                           \
        hipError_t e_ = allow_big_lds(dense_wgrad_x6_dma_kernel<false, false, 0, 1, true>, WG_RING_BYTES);            \
        if (e_ != hipSuccess) return (int)e_;                                                                         \
        hipLaunchKernelGGL((dense_wgrad_x6_dma_kernel<false, false, 0, 1, true>), dim3(tm.grid()), dim3(DX6_THREADS),  \
                           WG_RING_BYTES, st, dY, ldd, X, ldx, ws, M, Kf, N, nchunk, tm, bt, dy_stride, vg, va, atile, hs); \
        return (int)hipGetLastError();                                                                                \
    }                                                                                                                 \
    }

#define TVAE_WGW_LAUNCH_DEF(NP_)                                                                                      \
    namespace tvae {                                                                                                  \
    int dense_wgrad_x6_wide_p##NP_(TVAE_WGW_LAUNCH_ARGS) {                                                            \
        if (M % WW_ROWS != 0 || Kf <= 128 || bt.tiles_per_batch <= 0 ||                                             \
            tm.tilesN != (Kf <= 160 ? 1 : cdiv(Kf, 192)))                                                             \
            return (int)hipErrorInvalidValue;                                                                         \
        const unsigned grid_ =                                                                                        \
            8u * cdiv(tm.splits * (tm.tilesM / bt.tiles_per_batch), 8) * bt.tiles_per_batch * tm.tilesN;              \
        if (Kf <= 160) {             /* five column groups: the 66-wide frame of the 50 x 50 geometry (132 columns) */ \
            hipError_t e_ = allow_big_lds(dense_wgrad_x6_wide_kernel<NP_, 5>, WW_RING_BYTES);                         \
            if (e_ != hipSuccess) return (int)e_;                                                                     \
            hipLaunchKernelGGL((dense_wgrad_x6_wide_kernel<NP_, 5>), dim3(grid_), dim3(DX6_THREADS), WW_RING_BYTES, st, \
                               dY, ldd, X, ldx, ws, M, Kf, N, nchunk, tm, bt, dy_stride, atile, hs);                  \
            return (int)hipGetLastError();                                                                            \
        }                                                                                                             \
        hipError_t e_ = allow_big_lds(dense_wgrad_x6_wide_kernel<NP_, 6>, WW_RING_BYTES);                             \
        if (e_ != hipSuccess) return (int)e_;                                                                         \
        hipLaunchKernelGGL((dense_wgrad_x6_wide_kernel<NP_, 6>), dim3(grid_), dim3(DX6_THREADS), WW_RING_BYTES, st,   \
                           dY, ldd, X, ldx, ws, M, Kf, N, nchunk, tm, bt, dy_stride, atile, hs);                      \
        return (int)hipGetLastError();                                                                                \
    }                                                                                                                 \
    }

#if TVAE_WG_NP == 1
TVAE_WG_LAUNCH_DEF(1)
TVAE_WG_LAUNCH_DEF_ABF
#elif TVAE_WG_NP == 2
TVAE_WG_LAUNCH_DEF(2)
TVAE_WGW_LAUNCH_DEF(2)
#elif TVAE_WG_NP == 3
TVAE_WG_LAUNCH_DEF(3)
TVAE_WGW_LAUNCH_DEF(3)
#else
#error "dense_wgrad_x6_instance.hip is compiled once per number of parts: -DTVAE_WG_NP=1, 2 or 3"
#endif
