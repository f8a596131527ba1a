// libtvae_cluster.so: C ABI of the CTF in the template (include/tvae_cluster.h, section "CTF in the template"): the norm of the
// CTF-filtered template per (image, slot, angle) and the weighted per-class sums of H^2.  Stateless like the other entry
// points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "ctf_pose_kernels.hpp"

using namespace tvae_cluster;

// the range of tvae_pose_classify without S, and one workgroup per (image, slot, angle)
static bool tcp_shape_ok(long N, long C, long n, long M, long A) {
    return refine_shape_ok(N, C, n, A, 0) && M >= 1 && M <= TCP_M_MAX && N * M * (2 * A + 1) <= GRID_MAX;
}
static long spec_tiles(long n) { return (n * half_side((int)n) + CTF_THREADS - 1) / CTF_THREADS; }

extern "C" {

long tvae_template_ctf_power_ws_floats(int N, int C, int n, int M, int A) { return tcp_shape_ok(N, C, n, M, A) ? 2 : 0; }

int tvae_template_ctf_power(const float* theta, const float* dx, const int* cand, const float* ref, const double* coef,
                            float* ppc, float* ws, long ws_floats, int N, int C, int n, int K, int M, int A, float t_scale,
                            float dtheta, float mask_radius, float mask_edge, tvae_stream_t stream) {
    if (!tcp_shape_ok(N, C, n, M, A) || K < 1 || K > CLASSES_MAX) return (int)hipErrorInvalidValue;
    if (!theta || !dx || !cand || !ref || !coef || !ppc || !ws) return (int)hipErrorInvalidValue;
    if (!aligned8(coef) || !aligned8(ws) || ws_floats < 2) return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f) || !finite(dtheta)) return (int)hipErrorInvalidValue;
    if (!mask_ok(mask_radius, mask_edge)) return (int)hipErrorInvalidValue;
    const long NA = 2L * A + 1;
    const size_t f = sizeof(float), Ns = (size_t)N;
    const Span in[] = {{theta, Ns * f}, {dx, 2 * Ns * f}, {cand, Ns * M * f}, {ref, (size_t)K * C * n * n * f},
                       {coef, 5 * Ns * sizeof(double)}};
    const Span out[] = {{ppc, Ns * M * NA * f}, {ws, 2 * f}};
    if (!outputs_clear(out, in)) return (int)hipErrorInvalidValue;
    static_assert(REFINE_SIDE_MAX <= CTF_ONDIE_MAX, "both buffers of every supported n sit in LDS");
    const size_t lds = ctf_lds_bytes(n);
    const hipError_t e = allow_big_lds(template_ctf_power_kernel, lds);
    if (e != hipSuccess) return (int)e;
    template_ctf_power_kernel<<<(unsigned)((long)N * M * NA), CTF_THREADS, lds, S(stream)>>>(
        theta, dx, cand, ref, coef, ppc, C, n, K, M, A, t_scale, dtheta, mask_radius, mask_edge);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_ctf_power_entries(const double* coef, const int* img, const float* w, const int* seg, double* D, double* wsum,
                           int* counts, int N, int E, int K, int n, tvae_stream_t stream) {
    if (!coef || !img || !w || !seg || !D || !wsum || !counts || !aligned8(coef) || !aligned8(D) || !aligned8(wsum))
        return (int)hipErrorInvalidValue;
    if (N < 1 || N > PLANES_MAX || E < 1 || E > CPW_E_MAX || K < 1 || K > CLASSES_MAX || n < 2 || n > SIDE_MAX)
        return (int)hipErrorInvalidValue;
    const long tiles = spec_tiles(n), grid = (long)K * tiles;
    if (grid > GRID_MAX) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), d = sizeof(double), Es = (size_t)E, Ks = (size_t)K;
    const Span in[] = {{coef, 5 * (size_t)N * d}, {img, Es * f}, {w, Es * f}, {seg, (Ks + 1) * f}};
    const Span out[] = {{D, Ks * n * half_side(n) * d}, {wsum, Ks * d}, {counts, Ks * f}};
    if (!outputs_clear(out, in)) return (int)hipErrorInvalidValue;
    ctf_power_weighted_kernel<<<(unsigned)grid, CTF_THREADS, 0, S(stream)>>>(coef, img, w, seg, D, wsum, counts, N, E, n,
                                                                            (int)tiles);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
