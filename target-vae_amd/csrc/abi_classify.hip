// libtvae_cluster.so: C ABI of the reassignment against the class averages (include/tvae_cluster.h).  Stateless like the
// other entry points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "classify_kernels.hpp"

using namespace tvae_cluster;

// the range of tvae_pose_refine, and 1 <= M <= 64
static bool classify_shape_ok(long N, long M, long C, long n, long A, long S) {
    return N >= 1 && N <= PLANES_MAX && M >= 1 && M <= CLASSIFY_M_MAX && C >= 1 && C <= REFINE_C_MAX && n >= 2 &&
           n <= REFINE_SIDE_MAX && A >= 0 && A <= REFINE_A_MAX && S >= 0 && S <= REFINE_S_MAX;   // (N NA workgroups < 2^31)
}

// candidate poses of an (image, slot)
static long classify_cand(int A, int S) { return (2L * A + 1) * (2 * S + 1) * (2 * S + 1); }

// [lo, hi) of `count` four-byte words
struct ClassifyRange {
    size_t lo, hi;
};
static ClassifyRange range_of(const void* p, long count) {
    const size_t lo = reinterpret_cast<size_t>(p);
    return {lo, lo + (p ? 4 * (size_t)count : 0)};
}
static bool overlap(ClassifyRange a, ClassifyRange b) { return a.lo < b.hi && b.lo < a.hi; }

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
    return (long)N * (2 * (long)M * classify_cand(A, S) + 1);
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
    if (!finite(mask_radius) || !finite(mask_edge) || mask_edge < 0.f) return (int)hipErrorInvalidValue;
    const long table = (long)M * classify_cand(A, S), plane = (long)C * n * n;      // table: floats of num or pp of an image
    if (ws_floats < (long)N * (2 * table + 1)) return (int)hipErrorInvalidValue;
    const ClassifyRange in[5] = {range_of(Y, N * plane), range_of(theta, N), range_of(dx, 2L * N), range_of(cand, (long)N * M),
                                 range_of(ref, K * plane)};
    const ClassifyRange out[9] = {range_of(cls_out, N),       range_of(best, 4L * N),  range_of(theta_out, N),
                                  range_of(dx_out, 2L * N),   range_of(score, 2L * N * M), range_of(num, N * table),
                                  range_of(pp, N * table),    range_of(yy, N),         range_of(ws, (long)N * (2 * table + 1))};
    for (const ClassifyRange& o : out)
        for (const ClassifyRange& i : in)
            if (overlap(o, i)) return (int)hipErrorInvalidValue;
    // the tables are the caller's where it asks for them, the workspace's [num | pp | yy] otherwise
    float* numt = num ? num : ws;
    float* ppt = pp ? pp : ws + (long)N * table;
    float* yyt = yy ? yy : ws + 2L * N * table;
    hipStream_t s = tvae_cluster::S(stream);                  // (the shift radius hides the helper's name here)
    int rc = (int)hipErrorInvalidValue;
    switch (S) {
#define TVAE_CLASSIFY_CASE(SV)                                                                                          \
    case SV:                                                                                                            \
        rc = classify_launch<SV>(Y, theta, dx, cand, ref, numt, ppt, yyt, N, C, n, K, M, A, t_scale, dtheta,           \
                                 mask_radius, mask_edge, s);                                                            \
        break;
        TVAE_CLASSIFY_CASE(0)
        TVAE_CLASSIFY_CASE(1)
        TVAE_CLASSIFY_CASE(2)
        TVAE_CLASSIFY_CASE(3)
        TVAE_CLASSIFY_CASE(4)
        TVAE_CLASSIFY_CASE(5)
        TVAE_CLASSIFY_CASE(6)
        TVAE_CLASSIFY_CASE(7)
        TVAE_CLASSIFY_CASE(8)
#undef TVAE_CLASSIFY_CASE
    }
    if (rc != 0) return rc;
    classify_select_kernel<<<(unsigned)((N + REFINE_TILE - 1) / REFINE_TILE), REFINE_TILE, 0, s>>>(
        theta, dx, cand, numt, ppt, yyt, cls_out, theta_out, dx_out, score, best, N, n, K, M, A, S, t_scale, dtheta);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
