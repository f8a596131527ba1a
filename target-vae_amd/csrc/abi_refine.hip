// libtvae_cluster.so: C ABI of the pose refinement against the class averages (include/tvae_cluster.h).  Stateless like
// the other entry points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "refine_kernels.hpp"

using namespace tvae_cluster;

template <int S>
static int refine_launch(const float* Y, const float* theta, const float* dx, const int* cls, const float* ref, float* num,
                         float* pp, float* yy, int N, int C, int n, int K, int A, float t_scale, float dtheta,
                         float mask_radius, float mask_edge, hipStream_t s) {
    const size_t lds = refine_lds_floats(n, S) * sizeof(float);
    const hipError_t e = allow_big_lds(refine_corr_kernel<S>, lds);
    if (e != hipSuccess) return (int)e;
    refine_corr_kernel<S><<<(unsigned)((long)N * (2 * A + 1)), REFINE_TILE, lds, s>>>(
        Y, theta, dx, cls, ref, num, pp, yy, C, n, K, A, t_scale, dtheta, mask_radius, mask_edge);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

extern "C" {

long tvae_pose_refine_ws_floats(int N, int C, int n, int A, int S) {
    if (!refine_shape_ok(N, C, n, A, S)) return 0;
    return (long)N * (2 * refine_cand(A, S) + 1);
}

int tvae_pose_refine(const float* Y, const float* theta, const float* dx, const int* cls, const float* ref,
                     float* theta_out, float* dx_out, float* score, int* best, float* num, float* pp, float* yy, float* ws,
                     long ws_floats, int N, int C, int n, int K, int A, int S, float t_scale, float dtheta,
                     float mask_radius, float mask_edge, tvae_stream_t stream) {
    if (!refine_shape_ok(N, C, n, A, S) || K < 1 || K > CLASSES_MAX) return (int)hipErrorInvalidValue;
    if (!Y || !theta || !dx || !cls || !ref || !theta_out || !dx_out || !score || !best || !ws)
        return (int)hipErrorInvalidValue;
    if ((num == nullptr) != (pp == nullptr)) return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f) || !finite(dtheta)) return (int)hipErrorInvalidValue;
    if (!mask_ok(mask_radius, mask_edge)) return (int)hipErrorInvalidValue;
    const long cand = refine_cand(A, S), plane = (long)C * n * n;
    if (ws_floats < (long)N * (2 * cand + 1)) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), Ns = (size_t)N, table = Ns * cand * f;
    const Span in[] = {{Y, Ns * plane * f}, {theta, Ns * f}, {dx, 2 * Ns * f}, {cls, Ns * f}, {ref, (size_t)K * plane * f}};
    const Span out[] = {{theta_out, Ns * f}, {dx_out, 2 * Ns * f}, {score, 2 * Ns * f}, {best, 3 * Ns * f}, {num, table},
                        {pp, table}, {yy, Ns * f}, {ws, 2 * table + Ns * f}};
    if (!outputs_off_inputs(out, in)) return (int)hipErrorInvalidValue;
    // the tables are the caller's where it asks for them, the workspace's [num | pp | yy] otherwise
    float* numt = num ? num : ws;
    float* ppt = pp ? pp : ws + (long)N * cand;
    float* yyt = yy ? yy : ws + 2L * N * cand;
    hipStream_t s = tvae_cluster::S(stream);                  // (the shift radius hides the helper's name here)
    const int rc = refine_by_shift(S, [&](auto sv) {
        return refine_launch<decltype(sv)::value>(Y, theta, dx, cls, ref, numt, ppt, yyt, N, C, n, K, A, t_scale, dtheta,
                                                  mask_radius, mask_edge, s);
    });
    if (rc != 0) return rc;
    refine_select_kernel<<<(unsigned)((N + REFINE_TILE - 1) / REFINE_TILE), REFINE_TILE, 0, s>>>(
        theta, dx, cls, numt, ppt, yyt, theta_out, dx_out, score, best, N, n, K, A, S, t_scale, dtheta);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
