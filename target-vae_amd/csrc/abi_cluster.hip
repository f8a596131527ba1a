// libtvae_cluster.so: C ABI of the batched k-means kernels (include/tvae_cluster.h).  Stateless: no allocation, no
// synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "cluster_common.hpp"
#include "kmeans_kernels.hpp"

using namespace tvae_cluster;

// R <= 65535: the restarts are the y dimension of the launch grids
static bool shape_ok(long N, long d, long k, long R) {
    return d >= 1 && d <= 256 && k >= 1 && k <= 1024 && N >= 1 && k <= N && R >= 1 && R <= TVAE_KMEANS_MAX_RESTARTS &&
           R * N < (1L << 31);
}

extern "C" {

int tvae_cluster_abi_version(void) { return 1; }

int tvae_kmeans_groups(int N, int d, int k) { return shape_ok(N, d, k, 1) ? make_plan(N, d, k).G : 0; }

long tvae_kmeans_ws_floats(int N, int d, int k, int R) {
    return shape_ok(N, d, k, R) ? make_plan(N, d, k).per_restart * R : 0;
}

int tvae_kmeans_assign(const float* Xt, long ldx, const float* C, const int* done, int* labels, float* mind2,
                       int* changed, float* ws, long ws_floats, int N, int d, int k, int R, tvae_stream_t stream) {
    if (!shape_ok(N, d, k, R) || ldx < N || !Xt || !C || !done || !labels || !mind2 || !changed || !ws)
        return (int)hipErrorInvalidValue;
    const Plan pl = make_plan(N, d, k);
    if (ws_floats < pl.per_restart * R) return (int)hipErrorInvalidValue;
    const int vec = (ldx % 4 == 0) && ((reinterpret_cast<size_t>(Xt) & 15) == 0);
    const dim3 grid(pl.G, R);
    const size_t lds = (size_t)pl.KC * d * sizeof(float);
    hipStream_t s = S(stream);
    if (d <= 4)
        kmeans_assign_kernel<4><<<grid, TILE, lds, s>>>(Xt, ldx, C, done, labels, mind2, ws, N, d, k, pl, vec);
    else if (d <= 16)
        kmeans_assign_kernel<16><<<grid, TILE, lds, s>>>(Xt, ldx, C, done, labels, mind2, ws, N, d, k, pl, vec);
    else if (d <= 32)
        kmeans_assign_kernel<32><<<grid, TILE, lds, s>>>(Xt, ldx, C, done, labels, mind2, ws, N, d, k, pl, vec);
    else
        kmeans_assign_kernel<0><<<grid, TILE, lds, s>>>(Xt, ldx, C, done, labels, mind2, ws, N, d, k, pl, vec);
    TVAE_CLUSTER_CHECK_LAUNCH();
    kmeans_changed_sum_kernel<<<(R + 63) / 64, 64, 0, s>>>(ws, done, changed, d, k, R, pl);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_kmeans_update(const float* ws, long ws_floats, const int* done, float* C, float* inertia, float* shift,
                       int N, int d, int k, int R, tvae_stream_t stream) {
    if (!shape_ok(N, d, k, R) || !ws || !done || !C || !inertia || !shift) return (int)hipErrorInvalidValue;
    const Plan pl = make_plan(N, d, k);
    if (ws_floats < pl.per_restart * R) return (int)hipErrorInvalidValue;
    kmeans_update_kernel<<<R, TILE, 0, S(stream)>>>(ws, done, C, inertia, shift, d, k, pl);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_kmeans_mindist(const float* Xt, long ldx, const float* cnew, float* D, int N, int d, int R,
                        tvae_stream_t stream) {
    if (!shape_ok(N, d, 1, R) || ldx < N || !Xt || !cnew || !D) return (int)hipErrorInvalidValue;
    kmeans_mindist_kernel<<<dim3((unsigned)(((long)N + TILE - 1) / TILE), R), TILE, 0, S(stream)>>>(Xt, ldx, cnew, D, N, d);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
