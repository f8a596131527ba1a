// libtvae_hip.so, dense layers on the fp32 matrix pipe (gemm_f32_mfma.hpp): the 128-wide encoder 1x1x1
// layers in every arithmetic, and every dense layer when the caller asks for exact fp32 products.
#include "abi_common.hpp"
#include "gemm_f32_kernels.hpp"

using namespace tvae;

int tvae::splitk_finalize(const float* ws, int splits, int M, int N, const Epilogue& ep, hipStream_t stream) {
    int blocks = cdiv((long)M * N, 64);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(splitk_finalize_kernel, dim3(blocks), dim3(256), 0, stream, ws, splits, M, N, ep);
    return (int)hipGetLastError();
}

// ---- which kernels a call launches (tvae_linear_f32_route; the ids are listed in include/tvae_hip.h) ------------------------
// ONE plan for the launch and for the query, from shapes, leading dimensions, pointer ALIGNMENTS and the presence of the optional
// terms -- never from a pointer's value otherwise, so the query answers on a machine without a device.
enum { LIN_OP_FWD = 0, LIN_OP_DGRAD = 1, LIN_OP_WGRAD = 2 };
enum { LIN_GENERIC = 0, LIN_GLDS = 1, LIN_GLDS2 = 2, LIN_V4 = 3, LIN_NONE = 4 };
enum { LIN_F_GBIAS = 1, LIN_F_RES = 2, LIN_F_MASK = 4, LIN_F_ACC = 8 };
struct LinearPlan {
    int main;        // LIN_*: generic loaders | glds (fwd) | glds2 (dgrad) | V4 loaders (wgrad) | empty output, no launch
    int vec_ep;      // 1: tile_epilogue_v4 (glds / glds2 only), 0: tile_epilogue
    GemmSplit sp;    // generic / V4: slices and k-chunk of gemm_f32_kernel; glds / glds2: {1, K}
};

// align: bit i = the i-th POINTER argument of the entry point, in header order, is 16-byte aligned
//   fwd   W X bias gbias res Y   (ld_a = ldx, ld_b = ldy)        dgrad  W dpre add aux dX   (ld_a = ldd, ld_b = ldx)
//   wgrad dpre X dW ws           (ld_a = ldd, ld_b = ldx)
// the float4 epilogue needs plain row-major C (no per-image bias, no accumulate) and 16-B aligned C / residual / aux rows
static inline int vec_epilogue_ok(unsigned flags, long ldc, bool c_al, bool res_al, bool aux_al) {
    const bool plain = !(flags & LIN_F_GBIAS) && !(flags & LIN_F_ACC);
    const bool c_ok = c_al && ldc % 4 == 0;
    const bool r_ok = !(flags & LIN_F_RES) || (res_al && ldc % 4 == 0);       // (ldres == ldaux == ldc in both entry points)
    const bool a_ok = !(flags & LIN_F_MASK) || (aux_al && ldc % 4 == 0);
    return (plain && c_ok && r_ok && a_ok) ? 1 : 0;
}

static LinearPlan linear_plan(int op, int M, int N, int K, long ld_a, long ld_b, unsigned align, unsigned flags, long ws_floats) {
    auto al = [&](int i) { return ((align >> i) & 1u) != 0; };
    LinearPlan p{LIN_NONE, 0, {0, 0}};
    if (op == LIN_OP_FWD) {
        if (M <= 0 || N <= 0) return p;
        if (M % BM == 0 && N % BN == 0 && K % BK == 0 && ld_a % 4 == 0 && al(0) && al(1)) {
            // aligned shapes: the activation tile is staged by LDS-DMA (global_load_lds), the weight through registers
            p.main = LIN_GLDS; p.sp = {1, K};
            p.vec_ep = vec_epilogue_ok(flags & (LIN_F_GBIAS | LIN_F_RES), ld_b, al(5), al(4), true);
            return p;
        }
        p.main = LIN_GENERIC; p.sp = gemm_split_plan(M, N, K, 1, 0);
        return p;
    }
    if (op == LIN_OP_DGRAD) {
        if (K <= 0 || N <= 0) return p;
        if (K % BM == 0 && N % BN == 0 && M % BK == 0 && ld_a % 4 == 0 && al(0) && al(1)) {
            // both operands are row-contiguous along their tile dimension: A(kout, m) = W[m][kout], B = dpre[m][n]
            p.main = LIN_GLDS2; p.sp = {1, M};
            p.vec_ep = vec_epilogue_ok(flags & (LIN_F_RES | LIN_F_MASK), ld_b, al(4), al(2), al(3));
            return p;
        }
        p.main = LIN_GENERIC; p.sp = gemm_split_plan(K, N, M, 1, 0);
        return p;
    }
    if (M <= 0 || K <= 0) return p;
    const int tiles = cdiv(M, BM) * cdiv(K, BN);
    // V4: split-K chunks are multiples of BK, and N % BK == 0, so every k-step of every slice is full
    const bool v4 = M % BM == 0 && K % BN == 0 && N % BK == 0 && ld_a % 4 == 0 && ld_b % 4 == 0 && al(0) && al(1);
    p.main = v4 ? LIN_V4 : LIN_GENERIC;
    p.sp = gemm_split_plan(M, K, N, pick_splits(tiles, N), ws_floats);
    return p;
}

static inline unsigned abit(const void* p, int i) { return aligned16(p) ? (1u << i) : 0u; }

extern "C" {

int tvae_linear_f32_route(int op, int M, int N, int K, long ld_a, long ld_b, int align_mask, int flags, long ws_floats,
                          int which) {
    if (op < LIN_OP_FWD || op > LIN_OP_WGRAD) return -1;
    const LinearPlan p = linear_plan(op, M, N, K, ld_a, ld_b, (unsigned)align_mask, (unsigned)flags, ws_floats);
    return which == 0 ? p.main : which == 1 ? p.vec_ep : which == 2 ? p.sp.splits : -1;
}

int tvae_linear_fwd(const float* W, const float* X, const float* bias, const float* gbias, int group,
                    const float* res, float* Y, int M, int N, int K, long ldx, long ldy, int act, float slope,
                    tvae_stream_t stream) {
    const unsigned align = abit(W, 0) | abit(X, 1) | abit(bias, 2) | abit(gbias, 3) | abit(res, 4) | abit(Y, 5);
    const unsigned flags = (gbias ? LIN_F_GBIAS : 0) | (res ? LIN_F_RES : 0);
    const LinearPlan p = linear_plan(LIN_OP_FWD, M, N, K, ldx, ldy, align, flags, 0);
    if (p.main == LIN_NONE) return 0;
    Epilogue ep;
    ep.C = Y; ep.ldc = ldy;
    ep.bias = bias;
    ep.gbias = gbias; ep.ldg = M; ep.group = group > 0 ? group : 1;
    ep.res = res; ep.ldres = ldy;
    ep.act = act; ep.slope = slope;
    if (p.main == LIN_GLDS) {
        LoadKContigV4 af{W, (long)K, M};
        const TileMap tm{M / BM, N / BN, 1};
        hipLaunchKernelGGL((gemm_f32_glds_kernel<LoadKContigV4>), dim3(tm.grid()), dim3(GEMM_THREADS), 0, S(stream), af,
                           X, ldx, ep, M, N, K, tm, p.vec_ep);
        TVAE_CHECK_LAUNCH();
        return 0;
    }
    LoadKContig al{W, (long)K, M};
    LoadXContig bl{X, ldx, N};
    return (int)launch_gemm(al, bl, ep, M, N, K, p.sp, nullptr, S(stream));
}

int tvae_linear_dgrad(const float* W, const float* dpre, const float* add, const float* aux, float* dX, int M, int N,
                      int K, long ldd, long ldx, int mask, float slope, tvae_stream_t stream) {
    // dX[k][n] = sum_m W[m][k] dpre[m][n]: output rows = K, reduction = M
    const int emask = aux ? mask : ACT_NONE;
    const unsigned align = abit(W, 0) | abit(dpre, 1) | abit(add, 2) | abit(aux, 3) | abit(dX, 4);
    const unsigned flags = (add ? LIN_F_RES : 0) | (emask != ACT_NONE ? LIN_F_MASK : 0);
    const LinearPlan p = linear_plan(LIN_OP_DGRAD, M, N, K, ldd, ldx, align, flags, 0);
    if (p.main == LIN_NONE) return 0;
    Epilogue ep;
    ep.C = dX; ep.ldc = ldx;
    ep.res = add; ep.ldres = ldx;
    ep.aux = aux; ep.ldaux = ldx;
    ep.mask = emask; ep.slope = slope;
    if (p.main == LIN_GLDS2) {
        const TileMap tm{K / BM, N / BN, 1};
        hipLaunchKernelGGL(gemm_f32_glds2_kernel, dim3(tm.grid()), dim3(GEMM_THREADS), 0, S(stream), W, (long)K, dpre,
                           ldd, ep, K, N, M, tm, p.vec_ep);
        TVAE_CHECK_LAUNCH();
        return 0;
    }
    LoadXContig al{W, (long)K, K};
    LoadXContig bl{dpre, ldd, N};
    return (int)launch_gemm(al, bl, ep, K, N, M, p.sp, nullptr, S(stream));
}

int tvae_linear_wgrad(const float* dpre, const float* X, float* dW, float* ws, long ws_floats, int M, int N, int K,
                      long ldd, long ldx, int accumulate, tvae_stream_t stream) {
    // dW[m][k] = sum_n dpre[m][n] X[k][n]: output M x K, reduction = N
    const unsigned align = abit(dpre, 0) | abit(X, 1) | abit(dW, 2) | abit(ws, 3);
    const LinearPlan p = linear_plan(LIN_OP_WGRAD, M, N, K, ldd, ldx, align, accumulate ? LIN_F_ACC : 0, ws ? ws_floats : 0);
    if (p.main == LIN_NONE) return 0;
    Epilogue ep;
    ep.C = dW; ep.ldc = K;
    ep.accumulate = accumulate;
    if (p.main == LIN_V4) {
        LoadKContigV4 af{dpre, ldd, M};
        LoadKContigV4 bf{X, ldx, K};
        return (int)launch_gemm(af, bf, ep, M, K, N, p.sp, ws, S(stream));
    }
    LoadKContig al{dpre, ldd, M};
    LoadKContig bl{X, ldx, K};
    return (int)launch_gemm(al, bl, ep, M, K, N, p.sp, ws, S(stream));
}

}  // extern "C"
