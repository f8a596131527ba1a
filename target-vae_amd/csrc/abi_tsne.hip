// libtvae_cluster.so: C ABI of the t-SNE kernels (include/tvae_cluster.h).  Stateless like the k-means and Ward entry
// points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "cluster_common.hpp"
#include "tsne_kernels.hpp"

using namespace tvae_cluster;

static bool tsne_n_ok(long N) { return N >= 2 && N <= TSNE_N_MAX; }
static bool tsne_csr_ok(const int* rowptr, const int* col, const float* val, long nnz) {
    return rowptr && col && val && nnz >= 1 && nnz <= 0x7fffffffL;      // (the kernels take nnz as an int)
}

extern "C" {

int tvae_tsne_groups(int N) { return tsne_n_ok(N) ? tsne_plan(N).RT : 0; }

long tvae_tsne_repulsion_ws_floats(int N) {
    if (!tsne_n_ok(N)) return 0;
    const TsnePlan pl = tsne_plan(N);
    return 2L * pl.RT + 3L * pl.S * N;          // RT doubles first (the workspace must be 8-byte aligned)
}

int tvae_knn(const float* Xt, long ldx, int* idx, float* d2, int N, int d, int K, tvae_stream_t stream) {
    if (!tsne_n_ok(N) || d < 1 || d > 256 || K < 1 || K > KNN_K_MAX || K >= N || ldx < N || !Xt || !idx || !d2)
        return (int)hipErrorInvalidValue;
    const int rows = knn_rows(K), KC = knn_kc(d);
    const int vec = (ldx % 4 == 0) && ((reinterpret_cast<size_t>(Xt) & 15) == 0);
    const int grid = (N + rows - 1) / rows;
    const size_t lds = ((size_t)d * KC + 2 * (size_t)K * rows) * sizeof(float);
    hipStream_t s = S(stream);
    if (d <= 4)
        knn_kernel<4><<<grid, KNN_WAVE, lds, s>>>(Xt, ldx, idx, d2, N, d, K, rows, KC, vec);
    else if (d <= 16)
        knn_kernel<16><<<grid, KNN_WAVE, lds, s>>>(Xt, ldx, idx, d2, N, d, K, rows, KC, vec);
    else if (d <= 32)
        knn_kernel<32><<<grid, KNN_WAVE, lds, s>>>(Xt, ldx, idx, d2, N, d, K, rows, KC, vec);
    else
        knn_kernel<0><<<grid, KNN_WAVE, lds, s>>>(Xt, ldx, idx, d2, N, d, K, rows, KC, vec);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_tsne_repulsion(const float* Yt, long ldy, float* rep, double* Z, float* ws, long ws_floats, int N,
                        tvae_stream_t stream) {
    if (!tsne_n_ok(N) || ldy < N || !Yt || !rep || !Z || !ws || !aligned8(ws))
        return (int)hipErrorInvalidValue;
    const TsnePlan pl = tsne_plan(N);
    if (ws_floats < 2L * pl.RT + 3L * pl.S * N) return (int)hipErrorInvalidValue;
    double* zpart = reinterpret_cast<double*>(ws);
    float* part = ws + 2L * pl.RT;
    const int vec = (ldy % 4 == 0) && ((reinterpret_cast<size_t>(Yt) & 15) == 0);
    hipStream_t s = S(stream);
    tsne_repulsion_kernel<<<dim3(pl.RT, pl.S), TSNE_TILE, 0, s>>>(Yt, ldy, part, N, pl, vec);
    TVAE_CLUSTER_CHECK_LAUNCH();
    tsne_rows_kernel<<<pl.RT, TSNE_TILE, 0, s>>>(part, rep, ldy, zpart, N, pl.S);
    TVAE_CLUSTER_CHECK_LAUNCH();
    tsne_sum_kernel<<<1, TSNE_TILE, 0, s>>>(zpart, pl.RT, Z);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_tsne_step(const int* rowptr, const int* col, const float* val, long nnz, const float* Yt, const float* rep,
                   const double* Z, float* gains, float* update, float* Yt_out, float* grad, double* gnorm2, long ldy,
                   int N, float exaggeration, float momentum, float learning_rate, tvae_stream_t stream) {
    if (!tsne_n_ok(N) || ldy < N || !tsne_csr_ok(rowptr, col, val, nnz) || !Yt || !rep || !Z || !gains || !update ||
        !Yt_out || !gnorm2 || Yt_out == Yt)
        return (int)hipErrorInvalidValue;
    const int RT = tsne_plan(N).RT;
    tsne_step_kernel<<<RT, TSNE_TILE, 0, S(stream)>>>(rowptr, col, val, (int)nnz, Yt, rep, Z, gains, update,
                                                                 Yt_out, grad, gnorm2, ldy, N, exaggeration, momentum,
                                                                 learning_rate);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_tsne_kl(const int* rowptr, const int* col, const float* val, long nnz, const float* Yt, long ldy,
                 const double* Z, double* kl, double* ws, long ws_doubles, int N, tvae_stream_t stream) {
    if (!tsne_n_ok(N) || ldy < N || !tsne_csr_ok(rowptr, col, val, nnz) || !Yt || !Z || !kl || !ws)
        return (int)hipErrorInvalidValue;
    const int RT = tsne_plan(N).RT;
    if (ws_doubles < RT) return (int)hipErrorInvalidValue;
    hipStream_t s = S(stream);
    tsne_kl_kernel<<<RT, TSNE_TILE, 0, s>>>(rowptr, col, val, (int)nnz, Yt, ldy, Z, ws, N);
    TVAE_CLUSTER_CHECK_LAUNCH();
    tsne_sum_kernel<<<1, TSNE_TILE, 0, s>>>(ws, RT, kl);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
