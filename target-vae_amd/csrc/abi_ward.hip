// libtvae_cluster.so: C ABI of the Ward linkage kernels (include/tvae_cluster.h).  Stateless like the k-means entry points:
// no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "cluster_common.hpp"
#include "ward_kernels.hpp"

using namespace tvae_cluster;

static bool ward_shape_ok(long M, long d) { return M >= 2 && M <= WARD_M_MAX && d >= 1 && d <= 256; }

extern "C" {

int tvae_ward_nn_splits(int M, int d) { return ward_shape_ok(M, d) ? ward_plan(M, d).S : 0; }

long tvae_ward_nn_ws_floats(int M, int d) { return ward_shape_ok(M, d) ? 2L * ward_plan(M, d).S * M : 0; }

long tvae_ward_merge_ws_ints(int M, int d) { return ward_shape_ok(M, d) ? 2L * M : 0; }

int tvae_ward_nn(const float* Ct, long ldc, const float* cnt, int* nn, float* nd, float* ws, long ws_floats, int M,
                 int d, tvae_stream_t stream) {
    if (!ward_shape_ok(M, d) || ldc < M || !Ct || !cnt || !nn || !nd || !ws) return (int)hipErrorInvalidValue;
    const WardPlan pl = ward_plan(M, d);
    if (ws_floats < 2L * pl.S * M) return (int)hipErrorInvalidValue;
    float* pd = ws;
    int* pj = reinterpret_cast<int*>(ws + (long)pl.S * M);
    const int vec = (ldc % 4 == 0) && ((reinterpret_cast<size_t>(Ct) & 15) == 0);
    const dim3 grid(pl.RT, pl.S);
    const size_t lds = (size_t)pl.KC * (d + 1) * sizeof(float);
    hipStream_t s = S(stream);
    if (d <= 4)
        ward_nn_kernel<4><<<grid, WARD_TILE, lds, s>>>(Ct, ldc, cnt, pd, pj, M, d, pl, vec);
    else if (d <= 16)
        ward_nn_kernel<16><<<grid, WARD_TILE, lds, s>>>(Ct, ldc, cnt, pd, pj, M, d, pl, vec);
    else if (d <= 32)
        ward_nn_kernel<32><<<grid, WARD_TILE, lds, s>>>(Ct, ldc, cnt, pd, pj, M, d, pl, vec);
    else
        ward_nn_kernel<0><<<grid, WARD_TILE, lds, s>>>(Ct, ldc, cnt, pd, pj, M, d, pl, vec);
    TVAE_CLUSTER_CHECK_LAUNCH();
    ward_nn_reduce_kernel<<<pl.RT, WARD_TILE, 0, s>>>(pd, pj, nn, nd, M, pl.S);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

int tvae_ward_merge(const double* C_in, long ld_in, const float* cnt_in, const int* id_in, const double* hmax_in,
                    const int* nn, double* C_out, float* Ct_out, long ld_out, float* cnt_out, int* id_out,
                    double* hmax_out, int* rec_ids, double* rec_hs, int* m_out, int* ws, long ws_ints, int M, int d,
                    int N, int base, int cap, tvae_stream_t stream) {
    if (!ward_shape_ok(M, d) || ld_in < M || ld_out < M || N < M || N > WARD_M_MAX || base < 0 || cap < 0 ||
        (long)base + M / 2 > cap || ws_ints < 2L * M || !C_in || !cnt_in || !id_in || !hmax_in || !nn || !C_out ||
        !Ct_out || !cnt_out || !id_out || !hmax_out || !rec_ids || !rec_hs || !m_out || !ws)
        return (int)hipErrorInvalidValue;
    int* pos = ws;
    int* rank = ws + M;
    hipStream_t s = S(stream);
    ward_scan_kernel<<<1, WARD_SCAN, 0, s>>>(nn, pos, rank, m_out, M);
    TVAE_CLUSTER_CHECK_LAUNCH();
    const dim3 grid((M + WARD_TILE - 1) / WARD_TILE, d < WARD_FY ? d : WARD_FY);
    ward_apply_kernel<<<grid, WARD_TILE, 0, s>>>(C_in, ld_in, cnt_in, id_in, hmax_in, nn, pos, rank, C_out, Ct_out, ld_out,
                                                 cnt_out, id_out, hmax_out, rec_ids, rec_hs, M, d, N, base, cap);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
