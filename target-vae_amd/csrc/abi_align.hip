// libtvae_cluster.so: C ABI of the alignment, class-average, half-set and ring-correlation kernels
// (include/tvae_cluster.h).  Stateless like the k-means, Ward and t-SNE entry points: no allocation, no synchronisation,
// every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "align_kernels.hpp"
#include "class_stats_kernels.hpp"

using namespace tvae_cluster;

static bool align_shape_ok(long N, long C, long n) {
    if (N < 1 || N > PLANES_MAX || C < 1 || C > ALIGN_C_MAX || n < 2 || n > SIDE_MAX) return false;
    return N * C * align_tiles((int)n) <= GRID_MAX;        // workgroups of tvae_align_stack
}

static bool avg_shape_ok(long N, long K, long C, long n) {
    if (!align_shape_ok(N, C, n) || K < 1 || K > CLASSES_MAX) return false;
    return avg_slots((int)N, (int)K) * C * align_tiles((int)n) <= GRID_MAX;
}

// tvae_class_halves: three partial sums per slot and pixel; the slot count tripled where it bounds the grid
static bool halves_shape_ok(long N, long K, long C, long n) {
    if (!avg_shape_ok(N, K, C, n)) return false;
    return 3 * avg_slots((int)N, (int)K) * C * align_tiles((int)n) <= GRID_MAX;
}

// workspace of tvae_class_halves: (K + 1) cleaned boundaries and two member counts per slot (int32), padded to a multiple
// of 4 words, then the partial sums [slots][C][3][n][n]
static long halves_ws_ints(int N, int K) { return ((long)K + 1 + 2 * avg_slots(N, K) + 3) / 4 * 4; }

static bool frc_shape_ok(long P, long n) { return P >= 1 && P <= FRC_P_MAX && n >= 2 && n <= SIDE_MAX; }

// workspace: (K + 1) cleaned boundaries and one member count per slot (int32), padded to a multiple of 4 words, then the
// partial sums [slots][C][n][n]
static long avg_ws_ints(int N, int K) { return ((long)K + 1 + avg_slots(N, K) + 3) / 4 * 4; }

extern "C" {

long tvae_class_average_ws_floats(int N, int K, int C, int n) {
    if (!avg_shape_ok(N, K, C, n)) return 0;
    return avg_ws_ints(N, K) + avg_slots(N, K) * C * n * n;
}

int tvae_class_average_chunk(int N, int K, int C, int n) { return avg_shape_ok(N, K, C, n) ? AVG_CHUNK : 0; }

int tvae_align_stack(const float* Y, const float* theta, const float* dx, float* out, int N, int C, int n,
                     float t_scale, tvae_stream_t stream) {
    if (!align_shape_ok(N, C, n) || !Y || !theta || !dx || !out || out == Y) return (int)hipErrorInvalidValue;
    const int tiles = align_tiles(n);
    const unsigned grid = (unsigned)((long)N * C * tiles);
    align_stack_kernel<<<grid, ALIGN_TILE, 0, S(stream)>>>(Y, theta, dx, out, C, n, tiles, t_scale);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_class_average(const float* Y, const float* theta, const float* dx, const int* order, const int* seg, float* avg,
                       float* ws, long ws_floats, int N, int C, int n, int K, float t_scale, tvae_stream_t stream) {
    if (!avg_shape_ok(N, K, C, n) || !Y || !theta || !dx || !order || !seg || !avg || !ws)
        return (int)hipErrorInvalidValue;
    const long slots = avg_slots(N, K), ints = avg_ws_ints(N, K);
    if (ws_floats < ints + slots * C * n * n) return (int)hipErrorInvalidValue;
    int* clean = reinterpret_cast<int*>(ws);
    int* cnt = clean + (K + 1);
    float* part = ws + ints;
    const int tiles = align_tiles(n);
    hipStream_t s = S(stream);
    avg_seg_kernel<<<1, ALIGN_TILE, 0, s>>>(seg, clean, K, N);
    TVAE_CLUSTER_CHECK_LAUNCH();
    avg_accum_kernel<<<(unsigned)(slots * C * tiles), ALIGN_TILE, 0, s>>>(Y, theta, dx, order, clean, part, cnt, N, C, n,
                                                                         K, tiles, t_scale);
    TVAE_CLUSTER_CHECK_LAUNCH();
    avg_reduce_kernel<<<(unsigned)((long)K * C * tiles), ALIGN_TILE, 0, s>>>(part, cnt, clean, avg, C, n, tiles);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

long tvae_class_halves_ws_floats(int N, int K, int C, int n) {
    if (!halves_shape_ok(N, K, C, n)) return 0;
    return halves_ws_ints(N, K) + 3 * avg_slots(N, K) * C * n * n;
}

int tvae_class_halves(const float* Y, const float* theta, const float* dx, const int* order, const int* seg, float* avg,
                      float* half, float* var, int* counts, float* ws, long ws_floats, int N, int C, int n, int K,
                      float t_scale, tvae_stream_t stream) {
    if (!halves_shape_ok(N, K, C, n) || !Y || !theta || !dx || !order || !seg || !avg || !half || !var || !counts || !ws)
        return (int)hipErrorInvalidValue;
    const long slots = avg_slots(N, K), ints = halves_ws_ints(N, K);
    if (ws_floats < ints + 3 * slots * C * n * n) return (int)hipErrorInvalidValue;
    int* clean = reinterpret_cast<int*>(ws);
    int* cnt = clean + (K + 1);
    float* part = ws + ints;
    const int tiles = align_tiles(n);
    hipStream_t s = S(stream);
    avg_seg_kernel<<<1, ALIGN_TILE, 0, s>>>(seg, clean, K, N);
    TVAE_CLUSTER_CHECK_LAUNCH();
    halves_accum_kernel<<<(unsigned)(slots * C * tiles), ALIGN_TILE, 0, s>>>(Y, theta, dx, order, clean, part, cnt, N, C,
                                                                            n, K, tiles, t_scale);
    TVAE_CLUSTER_CHECK_LAUNCH();
    halves_reduce_kernel<<<(unsigned)((long)K * C * tiles), ALIGN_TILE, 0, s>>>(part, cnt, clean, avg, half, var, counts,
                                                                               K, C, n, tiles);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_frc_rings(int n) { return frc_shape_ok(1, n) ? half_side(n) : 0; }

long tvae_class_frc_ws_floats(int P, int n) { return frc_shape_ok(P, n) ? P * frc_plane_floats(n) : 0; }

int tvae_class_frc(const float* a, const float* b, float* frc, double* sums, float* ws, long ws_floats, int P, int n,
                   float mask_radius, float mask_edge, tvae_stream_t stream) {
    if (!frc_shape_ok(P, n) || !a || !b || !frc || !sums || !ws) return (int)hipErrorInvalidValue;
    if (!mask_ok(mask_radius, mask_edge)) return (int)hipErrorInvalidValue;
    if (ws_floats < P * frc_plane_floats(n) || !aligned8(ws)) return (int)hipErrorInvalidValue;
    const int H = half_side(n);
    float2* G = reinterpret_cast<float2*>(ws);                // [P][2][n][H] complex
    float* prod = ws + 4L * P * n * H;                        // [P][3][n][H]
    hipStream_t s = S(stream);
    frc_rows_kernel<<<dim3((n + FRC_ROWS - 1) / FRC_ROWS, P, 2), FRC_TILE, 0, s>>>(a, b, G, n, mask_radius, mask_edge);
    TVAE_CLUSTER_CHECK_LAUNCH();
    const long items = (long)((n + FRC_KY - 1) / FRC_KY) * H;
    frc_cols_kernel<<<dim3((unsigned)((items + FRC_TILE - 1) / FRC_TILE), P), FRC_TILE, 0, s>>>(G, prod, n);
    TVAE_CLUSTER_CHECK_LAUNCH();
    frc_rings_kernel<<<dim3((H + FRC_RING_TILE - 1) / FRC_RING_TILE, P), FRC_RING_TILE, 0, s>>>(prod, frc, sums, n);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
