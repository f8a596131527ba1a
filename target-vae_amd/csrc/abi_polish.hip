// libtvae_cluster.so: C ABI of the sub-pixel pose polish against the class averages (include/tvae_cluster.h).  Stateless like
// the other entry points: no allocation, no synchronisation; the state of the iteration lives in the caller's arrays.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "polish_kernels.hpp"

using namespace tvae_cluster;

extern "C" {

int tvae_pose_moments(const float* Y, const float* theta, const float* dx, const int* cls, const float* ref, float* mom, int N,
                      int C, int n, int K, float t_scale, float mask_radius, float mask_edge, tvae_stream_t stream) {
    if (!refine_shape_ok(N, C, n, 0, 0) || K < 1 || K > CLASSES_MAX) return (int)hipErrorInvalidValue;
    if (!Y || !theta || !dx || !cls || !ref || !mom) return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f)) return (int)hipErrorInvalidValue;
    if (!mask_ok(mask_radius, mask_edge)) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), Ns = (size_t)N, plane = (size_t)C * n * n * f;
    const Span in[] = {{Y, Ns * plane}, {theta, Ns * f}, {dx, 2 * Ns * f}, {cls, Ns * f}, {ref, (size_t)K * plane}};
    const Span out[] = {{mom, Ns * POLISH_MOMENTS * f}};
    if (!outputs_off_inputs(out, in)) return (int)hipErrorInvalidValue;
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
    if (!refine_shape_ok(N, 1, n, 0, 0) || K < 1 || K > CLASSES_MAX) return (int)hipErrorInvalidValue;
    if (!cls || !theta0 || !dx0 || !mom_try || !theta_try || !dx_try || !theta_out || !dx_out || !mom_cur || !score ||
        !lambda || !steps || !ended)
        return (int)hipErrorInvalidValue;
    if (!aligned8(lambda)) return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f)) return (int)hipErrorInvalidValue;
    if (!finite(max_shift) || max_shift < 0.f || !finite(max_angle) || max_angle < 0.f) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), Ns = (size_t)N, moments = Ns * POLISH_MOMENTS * f;
    const Span in[] = {{cls, Ns * f}, {theta0, Ns * f}, {dx0, 2 * Ns * f}, {mom_try, moments}};
    const Span out[] = {{theta_try, Ns * f}, {dx_try, 2 * Ns * f}, {theta_out, Ns * f}, {dx_out, 2 * Ns * f}, {mom_cur, moments},
                        {score, 2 * Ns * f}, {lambda, Ns * sizeof(double)}, {steps, Ns * f}, {ended, Ns * f}};
    if (!outputs_clear(out, in)) return (int)hipErrorInvalidValue;
    polish_step_kernel<<<(unsigned)((N + REFINE_TILE - 1) / REFINE_TILE), REFINE_TILE, 0, tvae_cluster::S(stream)>>>(
        cls, theta0, dx0, mom_try, theta_try, dx_try, theta_out, dx_out, mom_cur, score, lambda, steps, ended, N, n, K,
        first != 0, t_scale, max_shift, max_angle);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
