// libtvae_hip.so: the weight-gradient kernels of the split-pipe dense layers (dense_x6_kernels.hpp: dense_wgrad_x6_dma_kernel,
// dense_wgrad_x6_wide_kernel) for ONE number of parts, chosen on the command line (-DTVAE_WG_NP=1 | 2 | 3, set by the Makefile's
// pattern rule from the object's name), and their launchers.  1: one-part bf16 throughput mode, 2: h3 arithmetic (two fp16
// parts, three products), 3: exact three-part split.
#include "abi_dense_x6.hpp"

#if TVAE_WG_NP != 1 && TVAE_WG_NP != 2 && TVAE_WG_NP != 3
#error "dense_wgrad_x6_instance.hip is compiled once per number of parts: -DTVAE_WG_NP=1, 2 or 3"
#endif

namespace tvae {

// Sign bits against gy x the recomputed first-layer operand (WgVariant{true, true, WG_LRF_BITS}) runs in 32-column steps
// (STEP = 32, a ring of its own size) when the reduction slices and the images are multiples of 32 columns; -DTVAE_WG_STEP16
// keeps the 16-column instance everywhere (the A/B partner: profiles/tools/build_variant.sh dense_wgrad_x6_p2 -DTVAE_WG_STEP16
// old.so).
#ifdef TVAE_WG_STEP16
constexpr bool WG_STEP32 = false;
#else
constexpr bool WG_STEP32 = true;
#endif

// the eight admitted variants (abi_dense_x6.hpp: WgVariant), one instance of dense_wgrad_x6_dma_kernel<VIRT, XVA, LRF, NP> each
template <int NP>
int dense_wgrad_x6_launch(TVAE_WG_LAUNCH_ARGS) {
    auto go = [&](auto kernel, size_t ring) {
        return launch(kernel, dim3(tm.grid()), dim3(DX6_THREADS), ring, st, dY, ldd, X, ldx, ws, M, Kf, N, nchunk, tm, bt, dy_stride,
                      vg, va, atile, hs);
    };
    if (variant.lrf == WG_LRF_OFF) {
        if (variant.virt) {
            if (variant.xva) return go(dense_wgrad_x6_dma_kernel<true, true, 0, NP>, WG_RING_BYTES);
            return go(dense_wgrad_x6_dma_kernel<true, false, 0, NP>, WG_RING_BYTES);
        }
        if (variant.xva) return go(dense_wgrad_x6_dma_kernel<false, true, 0, NP>, WG_RING_BYTES);
        return go(dense_wgrad_x6_dma_kernel<false, false, 0, NP>, WG_RING_BYTES);
    }
    if (!variant.virt) return (int)hipErrorInvalidValue;     // the two-valued form IS a form of the implicit gradient operand
    if (variant.lrf == WG_LRF_H) {
        if (variant.xva) return go(dense_wgrad_x6_dma_kernel<true, true, 1, NP>, WG_RING_BYTES);
        return go(dense_wgrad_x6_dma_kernel<true, false, 1, NP>, WG_RING_BYTES);
    }
    if (!variant.xva) return go(dense_wgrad_x6_dma_kernel<true, false, 2, NP>, WG_RING_BYTES);
    if constexpr (WG_STEP32) {
        if (nchunk % 32 == 0 && N % 32 == 0 && va.Np >= 32 && va.Np % 32 == 0)
            return go(dense_wgrad_x6_dma_kernel<true, true, 2, NP, false, 32>, WG32_RING_BYTES);
    }
    return go(dense_wgrad_x6_dma_kernel<true, true, 2, NP>, WG_RING_BYTES);
}
template int dense_wgrad_x6_launch<TVAE_WG_NP>(TVAE_WG_LAUNCH_ARGS);

#if TVAE_WG_NP == 1
int dense_wgrad_x6_launch_abf(TVAE_WG_LAUNCH_ARGS) {
    if (variant.virt || variant.xva || variant.lrf != WG_LRF_OFF) return (int)hipErrorInvalidValue;
    return launch(dense_wgrad_x6_dma_kernel<false, false, 0, 1, true>, dim3(tm.grid()), dim3(DX6_THREADS), WG_RING_BYTES, st, dY,
                  ldd, X, ldx, ws, M, Kf, N, nchunk, tm, bt, dy_stride, vg, va, atile, hs);
}
#else
template <int NP>
int dense_wgrad_x6_wide(TVAE_WGW_LAUNCH_ARGS) {
    if (M % WW_ROWS != 0 || Kf <= 128 || bt.tiles_per_batch <= 0 || tm.tilesN != (Kf <= 160 ? 1 : cdiv(Kf, 192)))
        return (int)hipErrorInvalidValue;
    const unsigned grid = 8u * cdiv(tm.splits * (tm.tilesM / bt.tiles_per_batch), 8) * bt.tiles_per_batch * tm.tilesN;
    if (Kf <= 160)       // five column groups: the 66-wide frame of the 50 x 50 geometry (132 columns)
        return launch(dense_wgrad_x6_wide_kernel<NP, 5>, dim3(grid), dim3(DX6_THREADS), WW_RING_BYTES, st, dY, ldd, X, ldx, ws, M,
                      Kf, N, nchunk, tm, bt, dy_stride, atile, hs);
    return launch(dense_wgrad_x6_wide_kernel<NP, 6>, dim3(grid), dim3(DX6_THREADS), WW_RING_BYTES, st, dY, ldd, X, ldx, ws, M, Kf,
                  N, nchunk, tm, bt, dy_stride, atile, hs);
}
template int dense_wgrad_x6_wide<TVAE_WG_NP>(TVAE_WGW_LAUNCH_ARGS);
#endif

}  // namespace tvae
