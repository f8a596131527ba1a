// libtvae_hip.so, lifting convolution with exact fp32 products (conv_img_kernels.hpp: image-resident
// implicit GEMM on v_mfma_f32_32x32x2_f32; generic implicit-im2col loaders of the GEMM core when the padded image does
// not fit LDS).
#include "abi_common.hpp"
#include "conv_img_kernels.hpp"

using namespace tvae;

// LDS budget for the image-resident conv kernels (160 KiB per CU on gfx950; keep room for 1 workgroup).
static const size_t CONV_IMG_LDS_MAX = 150 * 1024;

// ---- which instance a call launches (tvae_conv1_f32_route; the ids are listed in include/tvae_hip.h) ---------------------
// ONE plan per entry point, host arithmetic on the geometry (and the workspace size) only: the launch executes it, the query
// reports it.  route < 0: the entry point refuses (hipErrorInvalidValue) before any launch.
enum { CONV_FWD_GENERIC = 0, CONV_FWD_IMG = 1, CONV_FWD_IMG_VEC = 2, CONV_FWD_IMG_VEC2 = 3 };
enum { CONV_WG_GENERIC = 0, CONV_WG_IMG_K16 = 1, CONV_WG_IMG_K32 = 2, CONV_WG_IMG_K32_N2 = 3 };

struct ConvFwdPlan {
    int route;               // CONV_FWD_*, -1: refused
    ConvGeom g;
    int sh;                  // log2 R
    int M, N, K;
    int rows, tilesPerImg;   // image-resident routes: padded-image rows per tile, position tiles per image
    size_t lds;
    unsigned grid;
};

static ConvFwdPlan conv_fwd_plan(int B, int Cin, int n, int ksz, int pad, int C, int R) {
    ConvFwdPlan p{};
    p.route = -1;
    p.g = make_geom(B, Cin, n, ksz, pad, R);
    const ConvGeom& g = p.g;
    if (g.Ho <= 0) return p;
    p.M = C * R; p.N = B * g.P; p.K = Cin * g.K2;
    int sh = 0; while ((1 << sh) < R) ++sh;
    if ((1 << sh) != R) return p;   // reference allows R in {4, 8, 16}
    p.sh = sh;
    p.rows = conv_fwd_img_rows(n, ksz, pad);
    p.lds = conv_img_lds_bytes(Cin, p.rows, n, pad);
    if (p.lds <= CONV_IMG_LDS_MAX) {
        // image-resident path: the padded-image rows of the tile in LDS, B fragments read straight from them
        p.tilesPerImg = cdiv(g.P, BN);
        const long nblk = (long)cdiv(p.M, BM) * B * p.tilesPerImg;
        if (nblk > 2147483647L) return p;
        const bool vec = (p.K % BK == 0) && (p.M % BM == 0);
        const size_t lds2 = conv_img_lds_bytes(Cin, p.rows, n, pad, 2);
        if (vec && p.M % (2 * BM) == 0 && lds2 <= CONV_IMG_LDS_MAX) {
            // 256 x 128 tile: each wave 128 x 64 (8 MFMAs per operand wait)
            p.route = CONV_FWD_IMG_VEC2;
            p.lds = lds2;
            p.grid = (unsigned)((long)(p.M / (2 * BM)) * B * p.tilesPerImg);
            return p;
        }
        p.route = vec ? CONV_FWD_IMG_VEC : CONV_FWD_IMG;
        p.grid = (unsigned)nblk;
        return p;
    }
    // generic path (padded image does not fit in LDS): implicit im2col staged through LDS
    p.route = CONV_FWD_GENERIC;
    return p;
}

struct ConvWgradPlan {
    int route;               // CONV_WG_*, -1: refused
    ConvGeom g;
    int M, N, K;
    int tiles;               // 128 x 128 output tiles
    // image-resident routes
    int tilesM, tilesNk;     // row tiles; tap tiles of the instance (256 taps wide for <1,32,2>)
    int rows;
    size_t lds;
    int sp, ips;             // image slices, images per slice
    // generic route
    GemmSplit split;
};

static ConvWgradPlan conv_wgrad_plan(int B, int Cin, int n, int ksz, int pad, int C, int R, long ws_floats) {
    ConvWgradPlan p{};
    p.route = -1;
    p.g = make_geom(B, Cin, n, ksz, pad, R);
    const ConvGeom& g = p.g;
    if (g.Ho <= 0) return p;
    if (R < 1 || (R & (R - 1)) != 0) return p;   // as the forward: the pair serves one layer (reference: R in {4, 8, 16})
    p.M = C * R; p.N = Cin * g.K2;
    const long Kl = (long)B * g.P;
    if (Kl > 2147483647L) return p;
    p.K = (int)Kl;
    const int M = p.M, N = p.N;
    const int tilesM = cdiv(M, BM), tilesN = cdiv(N, BN);
    p.tilesM = tilesM;
    p.tiles = tilesM * tilesN;
    const int rows = conv_wgrad_img_rows(Cin, n, ksz, pad);
    const size_t lds = conv_img_lds_bytes(Cin, rows, n, pad);
    if (lds <= CONV_IMG_LDS_MAX) {
        // image-resident path.  The image reduction is split into ~4 waves of resident workgroups: zero skipping makes
        // edge-tap tiles up to 2x lighter, and many smaller slices let the dispatcher balance that (sweep at cfg4:
        // 3 / 6 / 12 / 32 slices -> 20.4 / 20.1 / 19.65 / 19.7 ms)
        const long per = (long)M * N;
        const long cap = per > 0 ? ws_floats / per : 0;
        auto slices = [&](int out_tiles, int per_cu, int& ips) {
            int sp = (4 * 256 * per_cu + out_tiles / 2) / out_tiles;
            if (sp > B) sp = B;
            if (cap < 2) sp = 1; else if (sp > cap) sp = (int)cap;
            if (sp < 1) sp = 1;
            ips = cdiv(B, sp);
            return cdiv(B, ips);
        };
        // 128 x 256 tile (wave 64 x 128, 32 positions per k-step): every dY panel is re-read by half as many tap tiles
        const int rows2 = conv_wgrad_img_rows(Cin, n, ksz, pad, 2);
        const size_t ldsn = conv_img_lds_bytes(Cin, rows2, n, pad, 1, 32);
        const size_t lds32 = conv_img_lds_bytes(Cin, rows, n, pad, 1, 32);
        if (N % (2 * BN) == 0 && ldsn * 2 <= 160 * 1024) {
            p.route = CONV_WG_IMG_K32_N2;
            p.tilesNk = N / (2 * BN); p.rows = rows2; p.lds = ldsn;
            p.sp = slices(tilesM * p.tilesNk, 2, p.ips);
        } else if (lds32 * 3 <= 160 * 1024) {
            // 128 x 128 tile, 32 positions per k-step: half the barriers, still 3 workgroups per CU
            p.route = CONV_WG_IMG_K32;
            p.tilesNk = tilesN; p.rows = rows; p.lds = lds32;
            p.sp = slices(p.tiles, 3, p.ips);
        } else {
            p.route = CONV_WG_IMG_K16;
            p.tilesNk = tilesN; p.rows = rows; p.lds = lds;
            p.sp = slices(p.tiles, 3, p.ips);
        }
        return p;
    }
    p.route = CONV_WG_GENERIC;
    p.split = gemm_split_plan(M, N, p.K, pick_splits(p.tiles, p.K), ws_floats);
    return p;
}

extern "C" {

int tvae_conv1_f32_route(int B, int Cin, int n, int ksz, int pad, int C, int R, long ws_floats, int which) {
    if (which == 0) return conv_fwd_plan(B, Cin, n, ksz, pad, C, R).route;
    if (which < 0 || which > 3) return -1;
    const ConvWgradPlan p = conv_wgrad_plan(B, Cin, n, ksz, pad, C, R, ws_floats);
    if (p.route < 0) return -1;
    const bool gen = p.route == CONV_WG_GENERIC;
    return which == 1 ? p.route : which == 2 ? (gen ? p.split.splits : p.sp) : (gen ? 0 : p.ips);
}

int tvae_conv1_fwd(const float* y, const float* bank, const float* bias, float* out, int B, int Cin, int n, int ksz,
                   int pad, int C, int R, int act, float slope, tvae_stream_t stream) {
    const ConvFwdPlan p = conv_fwd_plan(B, Cin, n, ksz, pad, C, R);
    if (p.route < 0) return (int)hipErrorInvalidValue;
    const ConvGeom& g = p.g;
    const int M = p.M, N = p.N, K = p.K;
    Epilogue ep;
    ep.C = out; ep.ldc = (long)B * R * g.P;
    ep.bias = bias; ep.bias_shift = p.sh;
    ep.act = act; ep.slope = slope;
    ep.convR = R; ep.conv_shift = p.sh; ep.convP = g.P;
    switch (p.route) {
        case CONV_FWD_IMG_VEC2:
            return launch(conv1_fwd_img_kernel<true, 2>, dim3(p.grid), dim3(GEMM_THREADS), p.lds, S(stream), bank, y, g, ep, M, K,
                          p.tilesPerImg, p.rows);
        case CONV_FWD_IMG_VEC:
            return launch(conv1_fwd_img_kernel<true, 1>, dim3(p.grid), dim3(GEMM_THREADS), p.lds, S(stream), bank, y, g, ep, M, K,
                          p.tilesPerImg, p.rows);
        case CONV_FWD_IMG:
            return launch(conv1_fwd_img_kernel<false, 1>, dim3(p.grid), dim3(GEMM_THREADS), p.lds, S(stream), bank, y, g, ep, M, K,
                          p.tilesPerImg, p.rows);
        default: break;
    }
    LoadKContig al{bank, (long)K, M};
    LoadConvPatchFwd bl{y, g, N};
    return (int)launch_gemm(al, bl, ep, M, N, K, gemm_split_plan(M, N, K, 1, 0), nullptr, S(stream));
}

int tvae_conv1_wgrad(const float* y, const float* dpre, float* dbank, float* ws, long ws_floats, int B, int Cin,
                     int n, int ksz, int pad, int C, int R, tvae_stream_t stream) {
    const ConvWgradPlan p = conv_wgrad_plan(B, Cin, n, ksz, pad, C, R, ws ? ws_floats : 0);
    if (p.route < 0) return (int)hipErrorInvalidValue;
    const ConvGeom& g = p.g;
    const int M = p.M, N = p.N;
    Epilogue ep;
    ep.C = dbank; ep.ldc = N;
    if (p.route == CONV_WG_GENERIC) {
        LoadConvDY al{dpre, (long)B * R * g.P, M, R, g.P};
        LoadConvPatchWgrad bl{y, g, N};
        return (int)launch_gemm(al, bl, ep, M, N, p.K, p.split, ws, S(stream));
    }
    const dim3 grid((unsigned)(p.tilesM * p.tilesNk * p.sp));
    float* wsp = p.sp > 1 ? ws : nullptr;
    const long lddy = (long)B * R * g.P;
    int rc;
    if (p.route == CONV_WG_IMG_K32_N2)
        rc = launch(conv1_wgrad_img_kernel<1, 32, 2>, grid, dim3(GEMM_THREADS), p.lds, S(stream), dpre, lddy, y, g, ep, M, N,
                    p.ips, wsp, p.tilesNk, p.rows, p.sp, p.tilesM * p.sp);
    else if (p.route == CONV_WG_IMG_K32)
        rc = launch(conv1_wgrad_img_kernel<1, 32, 1>, grid, dim3(GEMM_THREADS), p.lds, S(stream), dpre, lddy, y, g, ep, M, N,
                    p.ips, wsp, p.tilesNk, p.rows, p.sp, p.tilesM * p.sp);
    else
        rc = launch(conv1_wgrad_img_kernel<1, 16, 1>, grid, dim3(GEMM_THREADS), p.lds, S(stream), dpre, lddy, y, g, ep, M, N,
                    p.ips, wsp, p.tilesNk, p.rows, p.sp, p.tilesM * p.sp);
    if (rc) return rc;
    return p.sp > 1 ? splitk_finalize(ws, p.sp, M, N, ep, S(stream)) : 0;
}

}  // extern "C"
