// libtvae_cluster.so: C ABI of the selection of a hard pose search from its tables (include/tvae_cluster.h).  Stateless like
// the other entry points: no allocation, no synchronisation, no workspace.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "pose_select_kernels.hpp"

using namespace tvae_cluster;

// the range of tvae_pose_classify (abi_classify.hip) without its channels, and the tables within 2^40 words
static bool select_shape_ok(long N, long n, long K, long M, long A, long S) {
    return refine_shape_ok(N, 1, n, A, S) && M >= 1 && M <= TVAE_CLASSIFY_MAX_CANDIDATES && K >= 1 && K <= CLASSES_MAX &&
           N * M * refine_cand((int)A, (int)S) < (1L << 40);
}

extern "C" {

int tvae_pose_select(const float* theta, const float* dx, const int* cand, const float* num, const float* pp, const float* yy,
                     int* cls_out, int* best, float* theta_out, float* dx_out, float* score, int N, int n, int K, int M, int A,
                     int S, int pp_per_shift, float t_scale, float dtheta, tvae_stream_t stream) {
    if (!select_shape_ok(N, n, K, M, A, S) || (pp_per_shift != 0 && pp_per_shift != 1)) return (int)hipErrorInvalidValue;
    if (!theta || !dx || !cand || !num || !pp || !yy || !cls_out || !best || !theta_out || !dx_out || !score)
        return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f) || !finite(dtheta)) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), Ns = (size_t)N, table = Ns * M * refine_cand(A, S) * f;
    const Span in[] = {{theta, Ns * f}, {dx, 2 * Ns * f}, {cand, Ns * M * f}, {num, table},
                       {pp, pp_per_shift ? table : Ns * M * (2 * (size_t)A + 1) * f}, {yy, Ns * f}};
    const Span out[] = {{cls_out, Ns * f}, {best, 4 * Ns * f}, {theta_out, Ns * f}, {dx_out, 2 * Ns * f}, {score, 2 * Ns * M * f}};
    if (!outputs_clear(out, in)) return (int)hipErrorInvalidValue;
    pose_select_kernel<<<(unsigned)((N + SELECT_IMAGES - 1) / SELECT_IMAGES), REFINE_TILE, 0, tvae_cluster::S(stream)>>>(
        theta, dx, cand, num, pp, yy, cls_out, best, theta_out, dx_out, score, N, n, K, M, A, S, pp_per_shift, t_scale, dtheta);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
