// libtvae_cluster.so: C ABI of the reassignment against the class averages (include/tvae_cluster.h).  Stateless like the
// other entry points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "classify_kernels.hpp"

using namespace tvae_cluster;

// the range of tvae_pose_refine, and 1 <= M <= 64
static bool classify_shape_ok(long N, long M, long C, long n, long A, long S) {
    return refine_shape_ok(N, C, n, A, S) && M >= 1 && M <= CLASSIFY_M_MAX;
}

template <int S>
static int classify_launch(const float* Y, const float* theta, const float* dx, const int* cand, const float* ref, float* num,
                           float* pp, float* yy, int N, int C, int n, int K, int M, int A, float t_scale, float dtheta,
                           float mask_radius, float mask_edge, hipStream_t s) {
    const size_t lds = classify_lds_floats(n, S) * sizeof(float);
    const hipError_t e = allow_big_lds(classify_corr_kernel<S>, lds);
    if (e != hipSuccess) return (int)e;
    classify_corr_kernel<S><<<(unsigned)((long)N * (2 * A + 1)), REFINE_TILE, lds, s>>>(
        Y, theta, dx, cand, ref, num, pp, yy, C, n, K, M, A, t_scale, dtheta, mask_radius, mask_edge);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

extern "C" {

long tvae_pose_classify_ws_floats(int N, int M, int C, int n, int A, int S) {
    if (!classify_shape_ok(N, M, C, n, A, S)) return 0;
    return (long)N * (2 * (long)M * refine_cand(A, S) + 1);
}

int tvae_pose_classify(const float* Y, const float* theta, const float* dx, const int* cand, const float* ref, int* cls_out,
                       int* best, float* theta_out, float* dx_out, float* score, float* num, float* pp, float* yy, float* ws,
                       long ws_floats, int N, int C, int n, int K, int M, int A, int S, float t_scale, float dtheta,
                       float mask_radius, float mask_edge, tvae_stream_t stream) {
    if (!classify_shape_ok(N, M, C, n, A, S) || K < 1 || K > CLASSES_MAX) return (int)hipErrorInvalidValue;
    if (!Y || !theta || !dx || !cand || !ref || !cls_out || !best || !theta_out || !dx_out || !score || !ws)
        return (int)hipErrorInvalidValue;
    if ((num == nullptr) != (pp == nullptr)) return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f) || !finite(dtheta)) return (int)hipErrorInvalidValue;
    if (!mask_ok(mask_radius, mask_edge)) return (int)hipErrorInvalidValue;
    const long table = (long)M * refine_cand(A, S), plane = (long)C * n * n;      // table: floats of num or pp of an image
    if (ws_floats < (long)N * (2 * table + 1)) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), Ns = (size_t)N, tables = Ns * table * f;
    const Span in[] = {{Y, Ns * plane * f}, {theta, Ns * f}, {dx, 2 * Ns * f}, {cand, Ns * M * f}, {ref, (size_t)K * plane * f}};
    const Span out[] = {{cls_out, Ns * f}, {best, 4 * Ns * f}, {theta_out, Ns * f}, {dx_out, 2 * Ns * f}, {score, 2 * Ns * M * f},
                        {num, tables}, {pp, tables}, {yy, Ns * f}, {ws, 2 * tables + Ns * f}};
    if (!outputs_off_inputs(out, in)) return (int)hipErrorInvalidValue;
    // the tables are the caller's where it asks for them, the workspace's [num | pp | yy] otherwise
    float* numt = num ? num : ws;
    float* ppt = pp ? pp : ws + (long)N * table;
    float* yyt = yy ? yy : ws + 2L * N * table;
    hipStream_t s = tvae_cluster::S(stream);                  // (the shift radius hides the helper's name here)
    const int rc = refine_by_shift(S, [&](auto sv) {
        return classify_launch<decltype(sv)::value>(Y, theta, dx, cand, ref, numt, ppt, yyt, N, C, n, K, M, A, t_scale, dtheta,
                                                    mask_radius, mask_edge, s);
    });
    if (rc != 0) return rc;
    classify_select_kernel<<<(unsigned)((N + REFINE_TILE - 1) / REFINE_TILE), REFINE_TILE, 0, s>>>(
        theta, dx, cand, numt, ppt, yyt, cls_out, theta_out, dx_out, score, best, N, n, K, M, A, S, t_scale, dtheta);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
