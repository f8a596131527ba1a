// Sub-pixel pose polish against the class averages (libtvae_cluster.so): the continuous step after the grid search of
// refine_kernels.hpp.  One evaluation renders ONE template per image -- that of tvae_pose_refine at A = 0, S = 0, position
// arithmetic, zero border, out-of-frame rule and mask included -- together with its derivatives along the two axes of the
// reference and along the angle, and reduces them to 15 sums per image; a thread per image then does the Levenberg-Marquardt
// bookkeeping in fp64 from those sums alone.  include/tvae_cluster.h states both definitions.  Included by abi_polish.hip only.
//
// polish_moments_kernel<STAGED>  a workgroup = one image, 256 threads.  Thread t takes the pixels t, t + 256, ... of channel 0,
//                        then of channel 1, ...: the image is read coalesced, once, and needs no LDS (there is no shift
//                        window).  The four taps of a pixel are gathered from the reference plane of the image's class:
//                        STAGED = true copies that plane into LDS first (n (n | 1) floats, odd row stride as refine_stride),
//                        false gathers from L2 as refine_build_template does.  The taps and so every output bit are the same.
//                        15 fmaf chains per thread, then a binary tree over 256 partial sums per moment.
// polish_step_kernel     a thread = an image: accept or reject the trial from its moments, the 4 x 4 normal equations of the
//                        next trial by Gaussian elimination with partial pivoting, the trust region.  fp64, contraction off:
//                        every product, sum and quotient is rounded on its own, in the order written here.
// No atomics; a sum's order depends on (n, C) only.
#pragma once
#include <hip/hip_runtime.h>

#include "refine_device.hpp"

// (fp contract stays off, as refine_device.hpp states it; said again so that this file does not lean on the include order)
#pragma clang fp contract(off)

namespace tvae_cluster {

constexpr int POLISH_MOMENTS = 15;
// mom[i][.]: the Gram sums of (P, Dtheta, G0, G1) in row-major upper-triangle order, the four sums against Y, and sum Y^2
enum PolishMoment {
    PM_PP, PM_PD, PM_PG0, PM_PG1, PM_DD, PM_DG0, PM_DG1, PM_G0G0, PM_G0G1, PM_G1G1, PM_PY, PM_DY, PM_G0Y, PM_G1Y, PM_YY
};

#ifndef TVAE_POLISH_STAGED
#define TVAE_POLISH_STAGED 1             // the reference plane through LDS (profiles/README.md has both timings)
#endif

// floats of LDS: the 15 x 256 partial sums, and the staged reference plane
static inline size_t polish_lds_floats(int n, bool staged) {
    return (size_t)POLISH_MOMENTS * REFINE_TILE + (staged ? (size_t)n * refine_stride(n) : 0);
}

// The bilinear sample of bilinear_zero_border (cluster_common.hpp; the same operations on the same taps, so `v` is that
// function's value bit for bit) and the derivatives of the SAME cell along the column and the row axis:
//     bc = (1 - wr) (a01 - a00) + wr (a11 - a10),   br = bot - top,
// exact 0 where the sample is the out-of-frame 0.  `stride` is the row stride of img (n in memory, n | 1 in LDS).
struct BilinearJet {
    float v, bc, br;
};
__device__ __forceinline__ BilinearJet bilinear_zero_border_jet(const float* __restrict__ img, int n, int stride, float col,
                                                                float row, bool in) {
    const float colc = in ? col : 0.f, rowc = in ? row : 0.f;
    const float fc = floorf(colc), fr = floorf(rowc);
    const int c0 = (int)fc, r0 = (int)fr;                     // in [-1, n - 1]
    const float wc = colc - fc, wr = rowc - fr;
    const bool c0in = c0 >= 0, c1in = c0 + 1 <= n - 1, r0in = r0 >= 0, r1in = r0 + 1 <= n - 1;
    const int ca = c0in ? c0 : 0, cb = c1in ? c0 + 1 : n - 1;
    const int ra = r0in ? r0 : 0, rb = r1in ? r0 + 1 : n - 1;
    const float v00 = img[ra * stride + ca], v01 = img[ra * stride + cb];
    const float v10 = img[rb * stride + ca], v11 = img[rb * stride + cb];
    const float a00 = (in && r0in && c0in) ? v00 : 0.f, a01 = (in && r0in && c1in) ? v01 : 0.f;
    const float a10 = (in && r1in && c0in) ? v10 : 0.f, a11 = (in && r1in && c1in) ? v11 : 0.f;
    const float dt = a01 - a00, db = a11 - a10;
    const float top = fmaf(wc, dt, a00);
    const float bot = fmaf(wc, db, a10);
    BilinearJet j;
    j.v = fmaf(wr, bot - top, top);
    j.bc = fmaf(wr, db - dt, dt);
    j.br = bot - top;
    return j;
}

// grid = N.  mom [N][15]
template <bool STAGED>
__global__ __launch_bounds__(REFINE_TILE) void polish_moments_kernel(
    const float* __restrict__ Y, const float* __restrict__ theta, const float* __restrict__ dx,
    const int* __restrict__ cls, const float* __restrict__ ref, float* __restrict__ mom, int C, int n, int K,
    float t_scale, float mask_radius, float mask_edge) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    float* __restrict__ mo = mom + (size_t)img * POLISH_MOMENTS;
    const int k = cls[img];
    if (k < 0 || k >= K) {                                    // uniform over the workgroup, before any barrier
        if (tid < POLISH_MOMENTS) mo[tid] = 0.f;
        return;
    }
    float* __restrict__ red = lds;                            // [15][REFINE_TILE]
    float* __restrict__ rs = lds + POLISH_MOMENTS * REFINE_TILE;   // [n][rstride], STAGED only
    const int rstride = STAGED ? refine_stride(n) : n;

    const RefinePose p = refine_angle_pose(theta, dx, img, 0, 0, t_scale, 0.f);
    const size_t nn = (size_t)n * n;
    const float step = 2.f / (float)(n - 1), half = 0.5f * (float)(n - 1);
    const bool masked = mask_radius > 0.f;

    float acc[POLISH_MOMENTS];
#pragma unroll
    for (int j = 0; j < POLISH_MOMENTS; ++j) acc[j] = 0.f;

    for (int ch = 0; ch < C; ++ch) {
        const float* __restrict__ Yp = Y + ((size_t)img * C + ch) * nn;
        const float* __restrict__ Rp = ref + ((size_t)k * C + ch) * nn;
        if (STAGED) {
            if (ch > 0) __syncthreads();                      // the previous channel's plane is still being read
            refine_load_plane(rs, Rp, n, rstride, tid);
            __syncthreads();
        }
        const float* __restrict__ plane = STAGED ? rs : Rp;
        for (int e = tid; e < n * n; e += REFINE_TILE) {
            const int r = e / n, q = e - r * n;
            const float y = Yp[e];
            const RefinePosition at = refine_position(q, r, step, half, p);
            const float u0 = at.u0, u1 = at.u1, col = at.col, row = at.row;
            const bool in = inside_frame(col, row, n);
            const BilinearJet b = bilinear_zero_border_jet(plane, n, rstride, col, row, in);
            float P = b.v, hc = mul_rn(half, b.bc), hr = mul_rn(half, b.br);
            if (masked) {
                const double d = sqrt((double)u0 * (double)u0 + (double)u1 * (double)u1) * (0.5 * (double)(n - 1));
                const float m = in ? soft_mask(d, mask_radius, mask_edge) : 0.f;
                P = in ? mul_rn(m, P) : 0.f;
                hc = mul_rn(m, hc);
                hr = mul_rn(m, hr);
            }
            // out of frame (a NaN or infinite u among it): exact zeros, never 0 * u
            const float g0 = in ? hc : 0.f;
            const float g1 = in ? -hr : 0.f;
            const float dt = in ? fmaf(u0, g1, -mul_rn(u1, g0)) : 0.f;
            acc[PM_PP] = fmaf(P, P, acc[PM_PP]);
            acc[PM_PD] = fmaf(P, dt, acc[PM_PD]);
            acc[PM_PG0] = fmaf(P, g0, acc[PM_PG0]);
            acc[PM_PG1] = fmaf(P, g1, acc[PM_PG1]);
            acc[PM_DD] = fmaf(dt, dt, acc[PM_DD]);
            acc[PM_DG0] = fmaf(dt, g0, acc[PM_DG0]);
            acc[PM_DG1] = fmaf(dt, g1, acc[PM_DG1]);
            acc[PM_G0G0] = fmaf(g0, g0, acc[PM_G0G0]);
            acc[PM_G0G1] = fmaf(g0, g1, acc[PM_G0G1]);
            acc[PM_G1G1] = fmaf(g1, g1, acc[PM_G1G1]);
            acc[PM_PY] = fmaf(P, y, acc[PM_PY]);
            acc[PM_DY] = fmaf(dt, y, acc[PM_DY]);
            acc[PM_G0Y] = fmaf(g0, y, acc[PM_G0Y]);
            acc[PM_G1Y] = fmaf(g1, y, acc[PM_G1Y]);
            acc[PM_YY] = fmaf(y, y, acc[PM_YY]);
        }
    }
#pragma unroll
    for (int j = 0; j < POLISH_MOMENTS; ++j) red[j * REFINE_TILE + tid] = acc[j];
    __syncthreads();
    for (int w = REFINE_TILE / 2; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int j = 0; j < POLISH_MOMENTS; ++j) red[j * REFINE_TILE + tid] += red[j * REFINE_TILE + tid + w];
        }
        __syncthreads();
    }
    if (tid < POLISH_MOMENTS) mo[tid] = red[tid * REFINE_TILE];
}

// ---- the step: fp64, a thread per image ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool polish_finite(double x) { return x - x == 0.0; }
__device__ __forceinline__ double dmul(double a, double b) { return a * b; }   // (contract off: never fused)
__device__ __forceinline__ double dadd(double a, double b) { return a + b; }
__device__ __forceinline__ double dsub(double a, double b) { return a - b; }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }

// the score of a pose from its moments: fp64 from the fp32 sums, NOT rounded to fp32 (near the optimum two poses differ by less
// than an fp32 step of the cosine); exactly 0 where pp or yy is 0
__device__ __forceinline__ double polish_score(const float* __restrict__ m) {
    if (m[PM_PP] == 0.f || m[PM_YY] == 0.f) return 0.0;
    return ddiv((double)m[PM_PY], __dsqrt_rn(dmul((double)m[PM_PP], (double)m[PM_YY])));
}

// The next trial of an image from the moments m of its current pose (th, d0, d1), the damping lam and the trust region around
// (ths, s0, s1) -> (tt, t0, t1); false = no step (the trial is the current pose bit for bit).
__device__ __forceinline__ bool polish_trial(const float* __restrict__ m, float th, float d0, float d1, float ths, float s0,
                                             float s1, double lam, int n, float t_scale, float max_shift, float max_angle,
                                             float& tt, float& t0, float& t1) {
    tt = th;
    t0 = d0;
    t1 = d1;
    const double pp = (double)m[PM_PP], py = (double)m[PM_PY];
    if (m[PM_PP] == 0.f || m[PM_YY] == 0.f) return false;
    // the correctly rounded fp32 cosine and sine (fp64, rounded once): a host restatement gets the same bits
    const double c = (double)(float)cos((double)th), s = (double)(float)sin((double)th);
    const double al = ddiv(py, pp);
    const double pd = (double)m[PM_PD], pg0 = (double)m[PM_PG0], pg1 = (double)m[PM_PG1], dd = (double)m[PM_DD];
    const double dg0 = (double)m[PM_DG0], dg1 = (double)m[PM_DG1], g00 = (double)m[PM_G0G0], g01 = (double)m[PM_G0G1];
    const double g11 = (double)m[PM_G1G1], dy = (double)m[PM_DY], g0y = (double)m[PM_G0Y], g1y = (double)m[PM_G1Y];
    // (Dtx, Dty) = (-c G0 - s G1, s G0 - c G1)
    const double px = dsub(-dmul(c, pg0), dmul(s, pg1)), pyy = dsub(dmul(s, pg0), dmul(c, pg1));
    const double dxm = dsub(-dmul(c, dg0), dmul(s, dg1)), dym = dsub(dmul(s, dg0), dmul(c, dg1));
    const double cc = dmul(c, c), ss = dmul(s, s), cs = dmul(c, s);
    const double xx = dadd(dadd(dmul(cc, g00), dmul(dmul(2.0, cs), g01)), dmul(ss, g11));
    const double xy = dadd(dsub(dmul(dsub(cc, ss), g01), dmul(cs, g00)), dmul(cs, g11));
    const double yyv = dadd(dsub(dmul(ss, g00), dmul(dmul(2.0, cs), g01)), dmul(cc, g11));
    const double xyv = dsub(-dmul(c, g0y), dmul(s, g1y)), yyy = dsub(dmul(s, g0y), dmul(c, g1y));
    const double a2 = dmul(al, al);
    // unknowns (dtheta, dtx, dty, dalpha): J = [al Dtheta, al Dtx, al Dty, P]
    double A[4][4], b[4];
    A[0][0] = dmul(a2, dd);
    A[0][1] = A[1][0] = dmul(a2, dxm);
    A[0][2] = A[2][0] = dmul(a2, dym);
    A[0][3] = A[3][0] = dmul(al, pd);
    A[1][1] = dmul(a2, xx);
    A[1][2] = A[2][1] = dmul(a2, xy);
    A[1][3] = A[3][1] = dmul(al, px);
    A[2][2] = dmul(a2, yyv);
    A[2][3] = A[3][2] = dmul(al, pyy);
    A[3][3] = pp;
    b[0] = dmul(al, dsub(dy, dmul(al, pd)));
    b[1] = dmul(al, dsub(xyv, dmul(al, px)));
    b[2] = dmul(al, dsub(yyy, dmul(al, pyy)));
    b[3] = dsub(py, dmul(al, pp));
#pragma unroll
    for (int i = 0; i < 4; ++i) A[i][i] = dadd(A[i][i], dmul(lam, A[i][i]));
    // Gaussian elimination, partial pivoting: the first row of the largest |A[r][k]|, r >= k
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        int piv = kk;
        double big = fabs(A[kk][kk]);
#pragma unroll
        for (int r = kk + 1; r < 4; ++r) {
            const double v = fabs(A[r][kk]);
            if (v > big) {
                big = v;
                piv = r;
            }
        }
#pragma unroll
        for (int r = kk + 1; r < 4; ++r) {
            if (piv == r) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double tmp = A[kk][j];
                    A[kk][j] = A[r][j];
                    A[r][j] = tmp;
                }
                const double tb = b[kk];
                b[kk] = b[r];
                b[r] = tb;
            }
        }
        const double pv = A[kk][kk];
        if (pv == 0.0 || !polish_finite(pv)) return false;
#pragma unroll
        for (int r = kk + 1; r < 4; ++r) {
            const double f = ddiv(A[r][kk], pv);
#pragma unroll
            for (int j = kk + 1; j < 4; ++j) A[r][j] = dsub(A[r][j], dmul(f, A[kk][j]));
            b[r] = dsub(b[r], dmul(f, b[kk]));
        }
    }
    double x[4];
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        double a = b[i];
#pragma unroll
        for (int j = i + 1; j < 4; ++j) a = dsub(a, dmul(A[i][j], x[j]));
        x[i] = ddiv(a, A[i][i]);
    }
    if (!polish_finite(x[0]) || !polish_finite(x[1]) || !polish_finite(x[2])) return false;
    // the new pose in fp64, clamped to the trust region, rounded to fp32 once; a rounding that leaves the region is taken back
    // by one fp32 step towards its centre
    const double ts = (double)t_scale;
    const double ra = (double)max_angle, rd = ddiv(ddiv(dmul((double)max_shift, 2.0), (double)(n - 1)), ts);
    const double cen[3] = {(double)ths, (double)s0, (double)s1};
    const double rad[3] = {ra, rd, rd};
    const double want[3] = {dadd((double)th, x[0]), dadd((double)d0, ddiv(x[1], ts)), dadd((double)d1, ddiv(x[2], ts))};
    const float cenf[3] = {ths, s0, s1};
    float out[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double lo = dsub(cen[i], rad[i]), hi = dadd(cen[i], rad[i]);
        double w = want[i];
        w = w < lo ? lo : w;
        w = w > hi ? hi : w;
        float f = (float)w;
        if (fabs(dsub((double)f, cen[i])) > rad[i]) f = nextafterf(f, cenf[i]);
        out[i] = f;
    }
    if (!refine_finite(out[0]) || !refine_finite(out[1]) || !refine_finite(out[2])) return false;
    tt = out[0];
    t0 = out[1];
    t1 = out[2];
    return true;
}

// grid = ceil(N / 256)
__global__ __launch_bounds__(REFINE_TILE) void polish_step_kernel(
    const int* __restrict__ cls, const float* __restrict__ theta0, const float* __restrict__ dx0,
    const float* __restrict__ mom_try, float* __restrict__ theta_try, float* __restrict__ dx_try,
    float* __restrict__ theta_out, float* __restrict__ dx_out, float* __restrict__ mom_cur, float* __restrict__ score,
    double* __restrict__ lambda, int* __restrict__ steps, int* __restrict__ ended, int N, int n, int K, int first,
    float t_scale, float max_shift, float max_angle) {
    const int i = blockIdx.x * REFINE_TILE + threadIdx.x;
    if (i >= N) return;
    const float* __restrict__ mt = mom_try + (size_t)i * POLISH_MOMENTS;
    float* __restrict__ mc = mom_cur + (size_t)i * POLISH_MOMENTS;
    const float ths = theta0[i], s0 = dx0[2 * (size_t)i], s1 = dx0[2 * (size_t)i + 1];
    float th, d0, d1;
    double lam;
    if (first) {
        const int k = cls[i];
        const double sd = polish_score(mt);
        const bool live = k >= 0 && k < K && polish_finite(sd);
        const float sc = (float)sd;
        th = ths;
        d0 = s0;
        d1 = s1;
        lam = 1e-3;
        theta_out[i] = th;
        dx_out[2 * (size_t)i] = d0;
        dx_out[2 * (size_t)i + 1] = d1;
        for (int j = 0; j < POLISH_MOMENTS; ++j) mc[j] = mt[j];
        score[2 * (size_t)i] = live ? sc : 0.f;
        score[2 * (size_t)i + 1] = live ? sc : 0.f;
        lambda[i] = lam;
        steps[i] = 0;
        if (!live) {
            theta_try[i] = th;
            dx_try[2 * (size_t)i] = d0;
            dx_try[2 * (size_t)i + 1] = d1;
            ended[i] = 1;
            return;
        }
    } else {
        if (ended[i]) return;
        th = theta_out[i];
        d0 = dx_out[2 * (size_t)i];
        d1 = dx_out[2 * (size_t)i + 1];
        lam = lambda[i];
        const double sd = polish_score(mt);
        if (polish_finite(sd) && sd > polish_score(mc)) {
            th = theta_try[i];
            d0 = dx_try[2 * (size_t)i];
            d1 = dx_try[2 * (size_t)i + 1];
            theta_out[i] = th;
            dx_out[2 * (size_t)i] = d0;
            dx_out[2 * (size_t)i + 1] = d1;
            for (int j = 0; j < POLISH_MOMENTS; ++j) mc[j] = mt[j];
            score[2 * (size_t)i + 1] = (float)sd;
            lam = ddiv(lam, 4.0);
            steps[i] = steps[i] + 1;
        } else {
            lam = dmul(lam, 8.0);
        }
        lambda[i] = lam;
    }
    float tt, t0, t1;
    polish_trial(mc, th, d0, d1, ths, s0, s1, lam, n, t_scale, max_shift, max_angle, tt, t0, t1);
    theta_try[i] = tt;
    dx_try[2 * (size_t)i] = t0;
    dx_try[2 * (size_t)i + 1] = t1;
    const bool same = __float_as_int(tt) == __float_as_int(th) && __float_as_int(t0) == __float_as_int(d0) &&
                      __float_as_int(t1) == __float_as_int(d1);
    ended[i] = same ? 1 : 0;
}

}  // namespace tvae_cluster
