// libtvae_cluster.so: C ABI of the sub-pixel pose polish against the class averages (include/tvae_cluster.h).  Stateless like
// the other entry points: no allocation, no synchronisation; the state of the iteration lives in the caller's arrays.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "polish_kernels.hpp"

using namespace tvae_cluster;

// [lo, hi) of `count` words of `bytes` bytes
struct PolishRange {
    size_t lo, hi;
};
static PolishRange range_of(const void* p, long count, int bytes = 4) {
    const size_t lo = reinterpret_cast<size_t>(p);
    return {lo, lo + (size_t)bytes * (size_t)count};
}
static bool overlap(PolishRange a, PolishRange b) { return a.lo < b.hi && b.lo < a.hi; }

extern "C" {

int tvae_pose_moments(const float* Y, const float* theta, const float* dx, const int* cls, const float* ref, float* mom, int N,
                      int C, int n, int K, float t_scale, float mask_radius, float mask_edge, tvae_stream_t stream) {
    if (N < 1 || N > PLANES_MAX || C < 1 || C > REFINE_C_MAX || n < 2 || n > REFINE_SIDE_MAX || K < 1 || K > CLASSES_MAX)
        return (int)hipErrorInvalidValue;
    if (!Y || !theta || !dx || !cls || !ref || !mom) return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f)) return (int)hipErrorInvalidValue;
    if (!finite(mask_radius) || !finite(mask_edge) || mask_edge < 0.f) return (int)hipErrorInvalidValue;
    const long plane = (long)C * n * n;
    const PolishRange in[5] = {range_of(Y, N * plane), range_of(theta, N), range_of(dx, 2L * N), range_of(cls, N),
                               range_of(ref, K * plane)};
    const PolishRange out = range_of(mom, (long)N * POLISH_MOMENTS);
    for (const PolishRange& i : in)
        if (overlap(out, i)) return (int)hipErrorInvalidValue;
    constexpr bool STAGED = TVAE_POLISH_STAGED != 0;
    const size_t lds = polish_lds_floats(n, STAGED) * sizeof(float);
    const hipError_t e = allow_big_lds(polish_moments_kernel<STAGED>, lds);
    if (e != hipSuccess) return (int)e;
    polish_moments_kernel<STAGED><<<(unsigned)N, REFINE_TILE, lds, tvae_cluster::S(stream)>>>(
        Y, theta, dx, cls, ref, mom, C, n, K, t_scale, mask_radius, mask_edge);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_pose_polish_step(const int* cls, const float* theta0, const float* dx0, const float* mom_try, float* theta_try,
                          float* dx_try, float* theta_out, float* dx_out, float* mom_cur, float* score, double* lambda,
                          int* steps, int* ended, int N, int n, int K, int first, float t_scale, float max_shift,
                          float max_angle, tvae_stream_t stream) {
    if (N < 1 || N > PLANES_MAX || n < 2 || n > REFINE_SIDE_MAX || K < 1 || K > CLASSES_MAX) return (int)hipErrorInvalidValue;
    if (!cls || !theta0 || !dx0 || !mom_try || !theta_try || !dx_try || !theta_out || !dx_out || !mom_cur || !score ||
        !lambda || !steps || !ended)
        return (int)hipErrorInvalidValue;
    if (!aligned8(lambda)) return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f)) return (int)hipErrorInvalidValue;
    if (!finite(max_shift) || max_shift < 0.f || !finite(max_angle) || max_angle < 0.f) return (int)hipErrorInvalidValue;
    const PolishRange in[4] = {range_of(cls, N), range_of(theta0, N), range_of(dx0, 2L * N),
                               range_of(mom_try, (long)N * POLISH_MOMENTS)};
    const PolishRange out[9] = {range_of(theta_try, N), range_of(dx_try, 2L * N),
                                range_of(theta_out, N), range_of(dx_out, 2L * N),
                                range_of(mom_cur, (long)N * POLISH_MOMENTS), range_of(score, 2L * N),
                                range_of(lambda, N, 8), range_of(steps, N),
                                range_of(ended, N)};
    for (int a = 0; a < 9; ++a) {
        for (const PolishRange& i : in)
            if (overlap(out[a], i)) return (int)hipErrorInvalidValue;
        for (int b = a + 1; b < 9; ++b)
            if (overlap(out[a], out[b])) return (int)hipErrorInvalidValue;
    }
    polish_step_kernel<<<(unsigned)((N + REFINE_TILE - 1) / REFINE_TILE), REFINE_TILE, 0, tvae_cluster::S(stream)>>>(
        cls, theta0, dx0, mom_try, theta_try, dx_try, theta_out, dx_out, mom_cur, score, lambda, steps, ended, N, n, K,
        first != 0, t_scale, max_shift, max_angle);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
