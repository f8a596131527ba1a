// libtvae_cluster.so: C ABI of the alignment and class-average kernels (include/tvae_cluster.h).  Stateless like the
// k-means, Ward and t-SNE entry points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "align_kernels.hpp"

using namespace tvae_cluster;

#define ALIGN_CHECK_LAUNCH()                     \
    do {                                         \
        hipError_t e__ = hipGetLastError();      \
        if (e__ != hipSuccess) return (int)e__;  \
    } while (0)

static bool align_shape_ok(long N, long C, long n) {
    if (N < 1 || N > ALIGN_N_MAX || C < 1 || C > ALIGN_C_MAX || n < 2 || n > ALIGN_SIDE_MAX) return false;
    return N * C * align_tiles((int)n) <= 0x7fffffffL;        // workgroups of tvae_align_stack
}

static bool avg_shape_ok(long N, long K, long C, long n) {
    if (!align_shape_ok(N, C, n) || K < 1 || K > ALIGN_K_MAX) return false;
    return avg_slots((int)N, (int)K) * C * align_tiles((int)n) <= 0x7fffffffL;
}

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
    align_stack_kernel<<<grid, ALIGN_TILE, 0, (hipStream_t)stream>>>(Y, theta, dx, out, C, n, tiles, t_scale);
    ALIGN_CHECK_LAUNCH();
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
    hipStream_t s = (hipStream_t)stream;
    avg_seg_kernel<<<1, ALIGN_TILE, 0, s>>>(seg, clean, K, N);
    ALIGN_CHECK_LAUNCH();
    avg_accum_kernel<<<(unsigned)(slots * C * tiles), ALIGN_TILE, 0, s>>>(Y, theta, dx, order, clean, part, cnt, N, C, n,
                                                                         K, tiles, t_scale);
    ALIGN_CHECK_LAUNCH();
    avg_reduce_kernel<<<(unsigned)((long)K * C * tiles), ALIGN_TILE, 0, s>>>(part, cnt, clean, avg, C, n, tiles);
    ALIGN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
