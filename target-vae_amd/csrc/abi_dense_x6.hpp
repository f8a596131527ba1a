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

// ---- which instance of dense_x6_kernel a forward / data-gradient call takes (tvae_linear_fwd_x6, tvae_linear_dgrad_x6) ----------
// dense_x6_route decides it, and every refusal, from the operands that are given and the shape alone: it compares pointers
// against null (and a3 against its alignment), reads no memory and launches nothing -- the shape of dft_route in
// abi_conv_dft.hip.  The launcher acts on its answer and on nothing else, so a refused call has launched nothing.
enum { DENSE_REFUSED = -1, DENSE_EMPTY = -2 };         // DenseRoute.xv: invalid value | no rows or no columns, nothing to do
// h3 (parts == 2): where the bound of the streamed operand comes from
enum H3XBound {
    H3X_NONE = 0,          // no bound needed (other arithmetics; the exact 0 / 1 operand of the two-valued gradient)
    H3X_RECOMPUTED,        // the recomputed first-layer activation: its bound words are formed in the cell buffer's trailer first
                           // (h3_zero_slots, dec_l0_bound)
    H3X_CALLER,            // an operand streamed from memory: the caller's x_amax
};
struct DenseRoute {
    int xv, epi;           // an entry of dense_x6_instances.def, or xv < 0 (above)
    H3XBound xbound;
};
static inline DenseRoute dense_x6_route(const void* a3, const float* X, const Epilogue& ep, int rows, int N, int K, int parts,
                                        const ColDot& cd, const InTail& it, const VirtGrad& vg, const VirtAct& va,
                                        bool have_x_amax) {
    const DenseRoute refused{DENSE_REFUSED, 0, H3X_NONE};
    if ((cd.w || it.xr) && rows > DX6_ROWS) return refused;              // the fused tails need ONE row tile
    if (rows <= 0 || N <= 0) return DenseRoute{DENSE_EMPTY, 0, H3X_NONE};
    if (N % 128 != 0 || !aligned16(a3) || (parts != 1 && parts != 2 && parts != 3)) return refused;
    H3XBound xbound = H3X_NONE;
    if (parts == 2) {
        // h3 instances: the recomputed first-layer activation and the exact 0 / 1 operand of the two-valued gradient; an operand
        // streamed from memory needs its maximum from the caller: max |X| or an upper bound of it (one device word) -- e.g.
        // |cos| <= 1 for Fourier features, the first-layer bound for a stored coordinate layer, a row-sum bound for the output of
        // a layer (tvae/ops.py: _h3_bounds)
        if (va.xr) xbound = H3X_RECOMPUTED;
        else if (have_x_amax && !vg.wo && !vg.csum) xbound = H3X_CALLER;
        else if (!vg.csum) return refused;
    }
    // the recomputed operands need tiles inside one image and tables of <= 512 entries
    if ((va.xr && (K > 512 || va.Np % 128 != 0 || vg.wo || vg.csum)) || (vg.csum && (!vg.gy || vg.act != ACT_LRELU)) ||
        (it.bc && it.Np % 128 != 0) || (!va.xr && !X && !(vg.bits && vg.csum && vg.rpart)))
        return refused;
    const bool one_tile = rows == DX6_ROWS, whole_tiles = rows % DX6_ROWS == 0;
    const bool ld31 = ep.ldc * 8 * 4 < (1L << 31) && ep.ldaux * 8 * 4 < (1L << 31);      // 32-bit byte offsets of the lean stores
    const bool tail = cd.w || cd.bits;
    int xv = 0, epi = 0;
    if (vg.csum && vg.rpart && vg.bits) {                // two-valued gradient: operand and row sums from the stored sign bits
        if (K > DX6_ROWS || N % 32 != 0) return refused;
        xv = 5;
        // the hot shape has its own lean instance: ONE full row tile, result not stored, fused first-layer backward with the
        // recomputed LeakyReLU mask, nothing else switched on
        if (one_tile && !ep.C && it.xr && it.bc && !ep.res && ep.mask == ACT_LRELU && !tail) epi = 2;
        // ... its result stored under the LeakyReLU mask of a saved activation (Fourier decoders), whole row tiles: lean store
        else if (whole_tiles && ep.C && !it.xr && !ep.res && ep.mask == ACT_LRELU && ep.aux && !tail && !ep.ctile && ld31) epi = 3;
    } else if (vg.csum && vg.rpart) {                    // ... streaming the saved activation, with its row sums
        if (K > DX6_ROWS) return refused;                // the row sums live in one 512-row LDS table
        xv = 4;
    } else if (vg.csum) {                                // ... without them
        xv = 3;
    } else if (va.xr) {                                  // streamed operand recomputed from the coordinates
        xv = 2;
        // forward of the decoder's last hidden layer with its activation not stored: lean instance (one full row tile)
        // (cd.bits == nullptr with no output either: the inference-mode forward -- only the fused column dot leaves the launch)
        if (one_tile && !ep.C && cd.w && !it.xr && !ep.res && ep.mask == ACT_NONE && ep.act == ACT_LRELU) epi = 1;
    } else if (vg.wo) {                                  // implicit gradient operand, general activation
        xv = 1;
    } else if (one_tile && !ep.C && cd.w && !it.xr && !ep.res && ep.mask == ACT_NONE && ep.act == ACT_LRELU) {
        epi = 1;         // the same layer with its input read from memory (28 x 28 shapes, Fourier decoders)
    } else if (whole_tiles && ep.C && !ep.res && !tail && !it.xr && !ep.ctile && !ep.accumulate && !ep.gbias && ld31 &&
               ((ep.mask == ACT_NONE && (ep.act == ACT_LRELU || ep.act == ACT_NONE)) ||
                (ep.mask == ACT_LRELU && ep.aux && ep.act == ACT_NONE && !ep.bias))) {
        // plain hidden layer that stores its output (round 6): whole 512-row tiles, bias + LeakyReLU | none (forward) or the
        // LeakyReLU mask of the saved activation (data gradient), nothing fused behind it: lean store epilogue
        epi = 3;
    }
    if (ep.amax_out && epi != 0 && epi != 3) return refused;             // only EPI 0 and 3 flush max |stored value|
    return DenseRoute{xv, epi, xbound};
}

// What the weight-gradient kernel streams (the template arguments VIRT, XVA, LRF of dense_wgrad_x6_dma_kernel).  Eight
// combinations have an instance: every (virt, xva) without the two-valued form, and virt with either two-valued form.
enum WgTwoValued { WG_LRF_OFF = 0, WG_LRF_H = 1, WG_LRF_BITS = 2 };     // 0 / 1 operand from the saved activation | its sign bits
struct WgVariant {
    bool virt;             // the gradient operand is given implicitly (VirtGrad.wo)
    bool xva;              // X is recomputed from the coordinates (VirtAct.xr)
    WgTwoValued lrf;       // the implicit LeakyReLU gradient in its two-valued form
};
constexpr WgVariant WG_PLAIN = {false, false, WG_LRF_OFF};

// weight-gradient launchers, one object per number of parts (dense_wgrad_x6_instance.hip)
#define TVAE_WG_LAUNCH_ARGS                                                                                           \
    const WgVariant &variant, const float *dY, long ldd, const float *X, long ldx, float *ws, int M, int Kf, int N,   \
        int nchunk, const TileMap &tm, const DenseBatch &bt, long dy_stride, const VirtGrad &vg, const VirtAct &va,   \
        const ATile &atile, hipStream_t st, const H3Scale &hs
template <int NP>
TVAE_INTERNAL int dense_wgrad_x6_launch(TVAE_WG_LAUNCH_ARGS);
// one-part mode with the A operand STORED as bf16 (dense_wgrad_x6_dma_kernel<.., ABF>)
TVAE_INTERNAL int dense_wgrad_x6_launch_abf(TVAE_WG_LAUNCH_ARGS);

// the exact-fit 256 x 192 tile of the spectral weight gradient (dense_wgrad_x6_wide_kernel; tm / bt count 256-row tiles):
// two and three parts only
#define TVAE_WGW_LAUNCH_ARGS                                                                                          \
    const float *dY, long ldd, const float *X, long ldx, float *ws, int M, int Kf, int N, int nchunk, const TileMap &tm, \
        const DenseBatch &bt, long dy_stride, const ATile &atile, hipStream_t st, const H3Scale &hs
template <int NP>
TVAE_INTERNAL int dense_wgrad_x6_wide(TVAE_WGW_LAUNCH_ARGS);

// pre-pass kernels that other units launch as well (dense_prepass_kernels.hpp, compiled in abi_dense_x6.hip alone): each launches
// and returns the error of the launch
TVAE_INTERNAL int h3_zero_slots(float* p, int n, int threads, hipStream_t st);
// (dense_split2h_rows_kernel for row-major operands of <= 48 k-octets: both sides coalesced through <= 48 KB of LDS)
TVAE_INTERNAL int dense_split2h(const float* W, long ldw, uint4* a3, int rows, int Rpad, int K, int K8pad, int transpose,
                                const float* scale, const float* rowmax, hipStream_t st);
// N columns (pixels) of xr [N][2]; nlb floats of lb (0: none)
TVAE_INTERNAL int dec_l0_bound(const float* xr, int N, const float* wc, const float* bc, const float* lb, long nlb, int K,
                               float* slots, hipStream_t st);

// The spectral contraction's own shape -- plain column-tiled output, whole tiles of `tile_rows` rows, nothing else switched on --
// has a lean store epilogue in all three batched launchers (round 6: the generic one took ~40 % of these launches).
// amax_excludes: a given ep.amax_out rules the lean instance out (dense_x6_batched: its generic instance flushes the maximum,
// EPI 4 never does; the kernels of the other two launchers are not wired for amax_out in either form).
static inline bool dense_x6_lean_store(const Epilogue& ep, int rows_per_problem, int tile_rows, bool amax_excludes) {
    return !ep.bias && !ep.res && !ep.aux && ep.act == ACT_NONE && ep.mask == ACT_NONE && ep.ctile > 0 && ep.C && !ep.accumulate &&
           !(amax_excludes && ep.amax_out) && rows_per_problem % tile_rows == 0 && ep.ldc * 8 * 4 < (1L << 31);
}

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
