// Host-side helpers shared by the translation units of libtvae_hip.so (one .hip file per kernel family, compiled in
// parallel).  Every __global__ function in the kernel headers has internal linkage: a template kernel is emitted where it is
// instantiated, a non-template one by EVERY unit that sees its definition -- so those sit in headers that one unit alone
// includes, and a kernel that several units launch has a TVAE_INTERNAL launcher in the unit that owns it.  Every kernel is thus
// built once (tests/test_host_cpu.py: test_every_kernel_is_built_once).
// The library keeps NO process-wide state: the arithmetic a call runs in is chosen by WHICH
// entry point the caller invokes (tvae_linear_fwd vs tvae_linear_fwd_x6, ...), never by a global mode.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "../../include/tvae_hip.h"
#include "gemm_f32_mfma.hpp"

#define TVAE_CHECK_LAUNCH()                      \
    do {                                         \
        hipError_t e__ = hipGetLastError();      \
        if (e__ != hipSuccess) return (int)e__;  \
    } while (0)

#define TVAE_INTERNAL __attribute__((visibility("hidden")))

namespace tvae {

static inline hipStream_t S(tvae_stream_t s) { return (hipStream_t)s; }
static inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }
static inline int grid1d(long total, int block, int cap = 8192) {
    long g = (total + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}
template <class KernelT>
static hipError_t allow_big_lds(KernelT kernel, size_t bytes) {
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}
// ONE launch: raises the kernel's dynamic-LDS limit where `lds` needs it, launches, returns the launch's error.  The arguments
// convert to the kernel's parameter types implicitly, as in a direct launch.
template <class KernelT, class... A>
static int launch(KernelT kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, A... args) {
    const hipError_t e = allow_big_lds(kernel, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return (int)hipGetLastError();
}
// A runtime number of parts (1: bf16 throughput mode, 2: h3, 3: exact split) as a compile-time constant:
//   by_parts(parts, [&](auto np) { return launch(some_kernel<np.value>, ...); })
// instantiates f for all THREE values, so it serves the kernels that exist in all three; by_flag does the same for a bool.
template <class F>
static int by_parts(int parts, F&& f) {
    switch (parts) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return (int)hipErrorInvalidValue;
    }
}
template <class F>
static int by_flag(bool on, F&& f) {
    return on ? f(std::true_type{}) : f(std::false_type{});
}
// number of split-K slices that brings a GEMM with `tiles` output tiles to ~4 workgroups per CU
static inline int pick_splits(int tiles, long K) {
    long want = (1024 + tiles - 1) / tiles;
    long maxs = K / (4 * BK);
    if (maxs < 1) maxs = 1;
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    return (int)want;
}
// Mid-size reductions (latent_bwd, dec_in_total_*, part_total_s1, dft_dbias_rows, enc_tail_wgrad_total): their <true>
// instances issue the loads of several terms of a sum together and then add them in the order of the one-load-at-a-time
// loops (<false>, the kernels as they were: TVAE_MIDSIZE_ILP=0).  Read at every call, so one process can run both.
static inline bool midsize_ilp() {
    const char* e = getenv("TVAE_MIDSIZE_ILP");
    return !(e && e[0] == '0');
}
static inline int panels_of(long N, int width) { return (int)((N + width - 1) / width); }

static inline ConvGeom make_geom(int B, int Cin, int n, int ksz, int pad, int R) {
    ConvGeom g;
    g.B = B; g.Cin = Cin; g.n = n; g.ksz = ksz; g.pad = pad; g.R = R;
    g.Ho = n + 2 * pad - ksz + 1;
    g.P = g.Ho * g.Ho;
    g.K2 = ksz * ksz;
    return g;
}

static const size_t X6_LDS_MAX = 160 * 1024;       // whole LDS of a CU (one workgroup per CU by design)

// splitk_finalize_kernel (compiled in abi_linear_f32.hip alone) over the M x N outputs of `splits` slabs; the launch's error
TVAE_INTERNAL int splitk_finalize(const float* ws, int splits, int M, int N, const Epilogue& ep, hipStream_t stream);

// Split-K of the generic GEMM, decided on the host from shapes and workspace alone (the launcher below and the route queries
// tvae_conv1_f32_route / tvae_linear_f32_route both read it): `splits_wanted` <= 1 means no split-K, `ws_floats` is the capacity
// of the workspace (0 without one); fewer than two slabs of M x N floats -> no split; k-chunks are whole k-steps, and the
// count is what those chunks need.  splits == 0: an empty output, nothing to launch.
struct GemmSplit {
    int splits, kchunk;
};
static inline GemmSplit gemm_split_plan(int M, int N, int K, int splits_wanted, long ws_floats) {
    if (M <= 0 || N <= 0) return {0, 0};
    int splits = splits_wanted < 1 ? 1 : splits_wanted;
    if (splits > 1) {
        const long per = (long)M * N;
        const long cap = ws_floats / per;
        if (cap < 2) splits = 1; else if (splits > cap) splits = (int)cap;
        if (splits > 65535) splits = 65535;
    }
    const int kchunk = cdiv(cdiv(K > 0 ? K : 1, splits), BK) * BK;
    return {cdiv(K > 0 ? K : 1, kchunk), kchunk};
}

// Host-side launcher of a planned generic GEMM (gemm_split_plan of the same M, N, K; ws: the workspace the plan counted).
template <class AL, class BL>
static hipError_t launch_gemm(AL al, BL bl, const Epilogue& ep, int M, int N, int K, const GemmSplit& sp, float* ws,
                              hipStream_t stream) {
    if (sp.splits < 1) return hipSuccess;
    const TileMap tm{cdiv(M, BM), cdiv(N, BN), sp.splits};
    float* wsp = sp.splits > 1 ? ws : nullptr;
    hipLaunchKernelGGL((gemm_f32_kernel<AL, BL>), dim3(tm.grid()), dim3(GEMM_THREADS), 0, stream, al, bl, ep, M, N, K,
                       sp.kchunk, wsp, tm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sp.splits > 1) e = (hipError_t)splitk_finalize(ws, sp.splits, M, N, ep, stream);
    return e;
}

}  // namespace tvae
