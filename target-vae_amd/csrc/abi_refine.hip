// libtvae_cluster.so: C ABI of the pose refinement against the class averages (include/tvae_cluster.h).  Stateless like
// the other entry points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "refine_kernels.hpp"

using namespace tvae_cluster;

static bool refine_shape_ok(long N, long C, long n, long A, long S) {
    return N >= 1 && N <= PLANES_MAX && C >= 1 && C <= REFINE_C_MAX && n >= 2 && n <= REFINE_SIDE_MAX && A >= 0 &&
           A <= REFINE_A_MAX && S >= 0 && S <= REFINE_S_MAX;      // (N NA workgroups: at most 2^24 * 65 < 2^31)
}

// candidates of an image
static long refine_cand(int A, int S) { return (2L * A + 1) * (2 * S + 1) * (2 * S + 1); }

// [lo, hi) of `count` four-byte words
struct RefineRange {
    size_t lo, hi;
};
static RefineRange range_of(const void* p, long count) {
    const size_t lo = reinterpret_cast<size_t>(p);
    return {lo, lo + (p ? 4 * (size_t)count : 0)};
}
static bool overlap(RefineRange a, RefineRange b) { return a.lo < b.hi && b.lo < a.hi; }

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
    if (!finite(mask_radius) || !finite(mask_edge) || mask_edge < 0.f) return (int)hipErrorInvalidValue;
    const long cand = refine_cand(A, S), plane = (long)C * n * n;
    if (ws_floats < (long)N * (2 * cand + 1)) return (int)hipErrorInvalidValue;
    const RefineRange in[5] = {range_of(Y, N * plane), range_of(theta, N), range_of(dx, 2L * N), range_of(cls, N),
                               range_of(ref, K * plane)};
    const RefineRange out[8] = {range_of(theta_out, N), range_of(dx_out, 2L * N), range_of(score, 2L * N),
                                range_of(best, 3L * N), range_of(num, N * cand), range_of(pp, N * cand),
                                range_of(yy, N),         range_of(ws, (long)N * (2 * cand + 1))};
    for (const RefineRange& o : out)
        for (const RefineRange& i : in)
            if (overlap(o, i)) return (int)hipErrorInvalidValue;
    // the tables are the caller's where it asks for them, the workspace's [num | pp | yy] otherwise
    float* numt = num ? num : ws;
    float* ppt = pp ? pp : ws + (long)N * cand;
    float* yyt = yy ? yy : ws + 2L * N * cand;
    hipStream_t s = tvae_cluster::S(stream);                  // (the shift radius hides the helper's name here)
    int rc = (int)hipErrorInvalidValue;
    switch (S) {
#define TVAE_REFINE_CASE(SV)                                                                                            \
    case SV:                                                                                                            \
        rc = refine_launch<SV>(Y, theta, dx, cls, ref, numt, ppt, yyt, N, C, n, K, A, t_scale, dtheta, mask_radius,     \
                               mask_edge, s);                                                                           \
        break;
        TVAE_REFINE_CASE(0)
        TVAE_REFINE_CASE(1)
        TVAE_REFINE_CASE(2)
        TVAE_REFINE_CASE(3)
        TVAE_REFINE_CASE(4)
        TVAE_REFINE_CASE(5)
        TVAE_REFINE_CASE(6)
        TVAE_REFINE_CASE(7)
        TVAE_REFINE_CASE(8)
#undef TVAE_REFINE_CASE
    }
    if (rc != 0) return rc;
    refine_select_kernel<<<(unsigned)((N + REFINE_TILE - 1) / REFINE_TILE), REFINE_TILE, 0, s>>>(
        theta, dx, cls, numt, ppt, yyt, theta_out, dx_out, score, best, N, n, K, A, S, t_scale, dtheta);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
