// libtvae_cluster.so: C ABI of the eigenimage kernels (include/tvae_cluster.h): the class covariance of the aligned,
// mean-subtracted members applied to a block of vectors, in two streaming passes that never write the aligned stack.
// Stateless like the other entry points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "eigen_kernels.hpp"

using namespace tvae_cluster;

// the range of tvae_class_average (abi_align.hip: its chunk is 32), J, and the grids of the launches here
static bool eigen_shape_ok(long N, long K, long C, long n, long J) {
    if (N < 1 || N > PLANES_MAX || C < 1 || C > EIGEN_C_MAX || n < 2 || n > SIDE_MAX) return false;
    if (K < 1 || K > CLASSES_MAX || J < 1 || J > EIGEN_J_MAX) return false;
    const long tiles = eigen_tiles((int)n);
    if (N * C * tiles > GRID_MAX || (N / 32 + K) * C * tiles > GRID_MAX) return false;
    return K * J * C * tiles <= GRID_MAX;                  // eigen_reduce_kernel; eigen_accum_kernel has fewer than the line above
}

// workspace of tvae_class_project: (K + 1) cleaned boundaries (int32, padded to a multiple of 4 words), then the mask [n][n]
static long project_ws_ints(int K) { return ((long)K + 1 + 3) / 4 * 4; }
// workspace of tvae_class_backproject: (K + 1) cleaned boundaries and one member count per slot (int32, padded to a multiple
// of 4 words), the mask [n][n], then the partial sums [slots][J][C][n][n]
static long backproject_ws_ints(int N, int K) { return ((long)K + 1 + eigen_slots(N, K) + 3) / 4 * 4; }

#define EIGEN_BY_J(J, LAUNCH)            \
    do {                                 \
        if ((J) == 1) { LAUNCH(1); }     \
        else if ((J) == 2) { LAUNCH(2); } \
        else if ((J) <= 4) { LAUNCH(4); } \
        else if ((J) <= 8) { LAUNCH(8); } \
        else { LAUNCH(16); }             \
    } while (0)

extern "C" {

long tvae_class_project_ws_floats(int N, int K, int C, int n, int J) {
    if (!eigen_shape_ok(N, K, C, n, J)) return 0;
    return project_ws_ints(K) + (long)n * n;
}

long tvae_class_backproject_ws_floats(int N, int K, int C, int n, int J) {
    if (!eigen_shape_ok(N, K, C, n, J)) return 0;
    return backproject_ws_ints(N, K) + (long)n * n + eigen_slots(N, K) * J * C * n * n;
}

int tvae_class_eigen_chunk(int N, int K, int C, int n, int J) { return eigen_shape_ok(N, K, C, n, J) ? EIGEN_CHUNK : 0; }

int tvae_class_project(const float* Y, const float* theta, const float* dx, const int* order, const int* seg,
                       const float* mean, const float* V, float* coef, float* norm2, float* ws, long ws_floats, int N, int C,
                       int n, int K, int J, float t_scale, float mask_radius, float mask_edge, tvae_stream_t stream) {
    if (!eigen_shape_ok(N, K, C, n, J) || !mask_ok(mask_radius, mask_edge)) return (int)hipErrorInvalidValue;
    if (!Y || !theta || !dx || !order || !seg || !mean || !V || !coef || !ws) return (int)hipErrorInvalidValue;
    const long ints = project_ws_ints(K), need = ints + (long)n * n;
    if (ws_floats < need || !aligned8(ws)) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), plane = (size_t)C * n * n * f;
    const Span out[] = {{coef, (size_t)N * J * f}, {norm2, (size_t)N * f}, {ws, (size_t)need * f}};
    const Span in[] = {{Y, N * plane}, {theta, N * f}, {dx, 2 * N * f}, {order, N * f}, {seg, ((size_t)K + 1) * f},
                       {mean, K * plane}, {V, (size_t)K * J * plane}};
    if (!outputs_clear(out, in)) return (int)hipErrorInvalidValue;
    int* clean = reinterpret_cast<int*>(ws);
    float* mask = ws + ints;
    hipStream_t s = S(stream);
    eigen_prep_kernel<<<1 + eigen_tiles(n), EIGEN_TILE, 0, s>>>(seg, clean, K, N, mask, n, mask_radius, mask_edge);
    TVAE_CLUSTER_CHECK_LAUNCH();
    const unsigned grid = (unsigned)((N + EIGEN_GROUP - 1) / EIGEN_GROUP);
#define LAUNCH(JT)                                                                                                   \
    eigen_project_kernel<JT><<<grid, EIGEN_TILE, 0, s>>>(Y, theta, dx, order, clean, mean, V, mask, coef, norm2, N, C, n, K, \
                                                         J, t_scale)
    EIGEN_BY_J(J, LAUNCH);
#undef LAUNCH
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_class_backproject(const float* Y, const float* theta, const float* dx, const int* order, const int* seg,
                           const float* mean, const float* coef, float* W, int* counts, float* ws, long ws_floats, int N,
                           int C, int n, int K, int J, float t_scale, float mask_radius, float mask_edge,
                           tvae_stream_t stream) {
    if (!eigen_shape_ok(N, K, C, n, J) || !mask_ok(mask_radius, mask_edge)) return (int)hipErrorInvalidValue;
    if (!Y || !theta || !dx || !order || !seg || !mean || !coef || !W || !counts || !ws) return (int)hipErrorInvalidValue;
    const long slots = eigen_slots(N, K), ints = backproject_ws_ints(N, K);
    const long need = ints + (long)n * n + slots * J * C * n * n;
    if (ws_floats < need || !aligned8(ws)) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), plane = (size_t)C * n * n * f;
    const Span out[] = {{W, (size_t)K * J * plane}, {counts, K * f}, {ws, (size_t)need * f}};
    const Span in[] = {{Y, N * plane}, {theta, N * f}, {dx, 2 * N * f}, {order, N * f}, {seg, ((size_t)K + 1) * f},
                       {mean, K * plane}, {coef, (size_t)N * J * f}};
    if (!outputs_clear(out, in)) return (int)hipErrorInvalidValue;
    int* clean = reinterpret_cast<int*>(ws);
    int* cnt = clean + (K + 1);
    float* mask = ws + ints;
    float* part = mask + (long)n * n;
    const int tiles = eigen_tiles(n);
    hipStream_t s = S(stream);
    eigen_prep_kernel<<<1 + tiles, EIGEN_TILE, 0, s>>>(seg, clean, K, N, mask, n, mask_radius, mask_edge);
    TVAE_CLUSTER_CHECK_LAUNCH();
    const unsigned grid = (unsigned)(slots * C * tiles);
#define LAUNCH(JT)                                                                                                   \
    eigen_accum_kernel<JT><<<grid, EIGEN_TILE, 0, s>>>(Y, theta, dx, order, clean, mean, coef, mask, part, cnt, N, C, n, K, \
                                                       J, tiles, t_scale)
    EIGEN_BY_J(J, LAUNCH);
#undef LAUNCH
    TVAE_CLUSTER_CHECK_LAUNCH();
    eigen_reduce_kernel<<<(unsigned)((long)K * J * C * tiles), EIGEN_TILE, 0, s>>>(part, cnt, clean, W, counts, C, n, J, tiles);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
