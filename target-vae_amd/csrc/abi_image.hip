// libtvae_cluster.so: C ABI of the particle-preprocessing kernels (include/tvae_cluster.h): the batched sandwich product of
// the Fourier downsample and the background-ring normalisation.  Stateless like the other entry points: no allocation, no
// synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "image_kernels.hpp"

using namespace tvae_cluster;

// groups of IMG_NORM_GROUP pixels per image
static long norm_groups(long n, long m) { return (n * m + IMG_NORM_GROUP - 1) / IMG_NORM_GROUP; }

static bool norm_shape_ok(long B, long n, long m) {
    if (B < 1 || B > PLANES_MAX || n < 1 || n > SIDE_MAX || m < 1 || m > SIDE_MAX) return false;
    return B * norm_groups(n, m) <= GRID_MAX;
}

extern "C" {

int tvae_image_resample(const float* X, const float* Ar, const float* Ai, const float* Br, const float* Bi, float* out,
                        int B, int H, int W, int r0, int c0, int M, int N, int m, int n, float scale,
                        tvae_stream_t stream) {
    if (!X || !Ar || !Br || !out || out == X || (Ai == nullptr) != (Bi == nullptr)) return (int)hipErrorInvalidValue;
    if (B < 1 || B > PLANES_MAX || M < 1 || M > SIDE_MAX || N < 1 || N > SIDE_MAX || m < 1 || m > M || n < 1 || n > N)
        return (int)hipErrorInvalidValue;
    if (H < 1 || W < 1 || r0 < 0 || c0 < 0 || (long)r0 + M > H || (long)c0 + N > W) return (int)hipErrorInvalidValue;
    const int nj = img_nj(n);
    const int tiles_m = img_cdiv(m, IMG_TM), tiles_n = img_cdiv(n, 64 * nj);
    const long grid = (long)B * tiles_m * tiles_n;
    if (grid > GRID_MAX) return (int)hipErrorInvalidValue;
    hipStream_t s = S(stream);
#define IMAGE_LAUNCH(NJ, IMAG)                                                                                          \
    image_resample_kernel<NJ, IMAG><<<(unsigned)grid, IMG_THREADS, 0, s>>>(X, Ar, Ai, Br, Bi, out, H, W, r0, c0, M, N, m, n, \
                                                                           scale, tiles_m, tiles_n)
    if (Ai) {
        if (nj == 2) IMAGE_LAUNCH(2, true); else IMAGE_LAUNCH(1, true);
    } else {
        if (nj == 2) IMAGE_LAUNCH(2, false); else IMAGE_LAUNCH(1, false);
    }
#undef IMAGE_LAUNCH
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

long tvae_image_normalize_ws_floats(int B, int n, int m) {
    return norm_shape_ok(B, n, m) ? 6L * B * norm_groups(n, m) : 0;
}

int tvae_image_normalize(const float* X, float* out, double* stats, float* ws, long ws_floats, int B, int n, int m,
                         float radius, tvae_stream_t stream) {
    if (!norm_shape_ok(B, n, m) || !X || !out || !stats || !ws) return (int)hipErrorInvalidValue;
    if (!finite(radius)) return (int)hipErrorInvalidValue;
    const int G = (int)norm_groups(n, m);
    if (ws_floats < 6L * B * G || !aligned8(ws) || !aligned8(stats))
        return (int)hipErrorInvalidValue;
    const double r = radius > 0.f ? (double)radius : 0.5 * (n < m ? n : m);
    const double r2 = r * r;
    double* part = reinterpret_cast<double*>(ws);
    const unsigned grid = (unsigned)((long)B * G);
    hipStream_t s = S(stream);
    image_norm_sum_kernel<<<grid, IMG_THREADS, 0, s>>>(X, part, n, m, G, r2);
    TVAE_CLUSTER_CHECK_LAUNCH();
    image_norm_dev_kernel<<<grid, IMG_THREADS, 0, s>>>(X, part, n, m, G, r2);
    TVAE_CLUSTER_CHECK_LAUNCH();
    image_norm_apply_kernel<<<grid, IMG_THREADS, 0, s>>>(X, out, stats, part, n, m, G);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
