// libtvae_cluster.so: C ABI of the maximum-likelihood class averages (include/tvae_cluster.h): the posterior over the
// candidates of tvae_pose_classify and the weighted aligned average over a list of entries.  Stateless like the other entry
// points: no allocation, no synchronisation, every size a pure function of the arguments.
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"
#include "ml2d_kernels.hpp"

using namespace tvae_cluster;

// the range of tvae_pose_classify (abi_classify.hip) without its channels, and P
static bool posterior_shape_ok(long N, long n, long K, long M, long A, long S, long P) {
    return refine_shape_ok(N, 1, n, A, S) && M >= 1 && M <= POST_M_MAX && K >= 1 && K <= CLASSES_MAX && P >= 1 &&
           P <= POST_KEEP_MAX;
}

// the range of tvae_class_average (abi_align.hip) with E entries in the place of its N members
static bool wavg_shape_ok(long E, long K, long C, long n) {
    if (E < 1 || E > WAVG_E_MAX || K < 1 || K > CLASSES_MAX || C < 1 || C > WAVG_C_MAX || n < 2 || n > SIDE_MAX) return false;
    return wavg_slots(E, (int)K) * C * wavg_tiles((int)n) <= GRID_MAX;
}
static bool wavg_stack_ok(long N, long C, long n) { return N >= 1 && N <= PLANES_MAX && N * C * wavg_tiles((int)n) <= GRID_MAX; }

// workspace: (K + 1) cleaned boundaries and one live count per slot (int32, padded to a multiple of 4 words), one fp64 weight
// sum per slot, then the partial sums [slots][C][n][n]
static long wavg_ws_ints(long E, int K) { return ((long)K + 1 + wavg_slots(E, K) + 3) / 4 * 4; }
static long wavg_ws_need(long E, int K, int C, int n) {
    const long slots = wavg_slots(E, K);
    return wavg_ws_ints(E, K) + 2 * slots + slots * C * n * n;
}

extern "C" {

int tvae_pose_posterior(const float* num, const float* pp, const float* yy, const int* cand, const double* logprior,
                        const float* theta, const float* dx, int* ent_idx, int* ent_cls, float* ent_theta, float* ent_dx,
                        float* ent_w, float* resp, double* lse, double* r2, float* kept, int N, int n, int K, int M, int A,
                        int S, int P, float t_scale, float dtheta, float sigma2, tvae_stream_t stream) {
    if (!posterior_shape_ok(N, n, K, M, A, S, P)) return (int)hipErrorInvalidValue;
    if (!num || !pp || !yy || !cand || !theta || !dx || !ent_idx || !ent_cls || !ent_theta || !ent_dx || !ent_w || !resp ||
        !lse || !r2 || !kept)
        return (int)hipErrorInvalidValue;
    if (!finite(t_scale) || !(t_scale > 0.f) || !finite(dtheta) || !finite(sigma2) || !(sigma2 > 0.f))
        return (int)hipErrorInvalidValue;
    if (!aligned8(lse) || !aligned8(r2) || !aligned8(logprior)) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), d = sizeof(double), Ns = (size_t)N;
    const size_t table = Ns * M * refine_cand(A, S) * f, ent = Ns * P * f;
    const Span in[] = {{num, table}, {pp, table}, {yy, Ns * f}, {cand, Ns * M * f}, {logprior, (size_t)K * d},
                       {theta, Ns * f}, {dx, 2 * Ns * f}};
    const Span out[] = {{ent_idx, ent}, {ent_cls, ent}, {ent_theta, ent}, {ent_dx, 2 * ent}, {ent_w, ent},
                        {resp, Ns * M * f}, {lse, Ns * d}, {r2, Ns * d}, {kept, Ns * f}};
    if (!outputs_clear(out, in)) return (int)hipErrorInvalidValue;
    posterior_kernel<<<(unsigned)N, POST_TILE, 0, tvae_cluster::S(stream)>>>(num, pp, yy, cand, logprior, theta, dx, ent_idx,
                                                                            ent_cls, ent_theta, ent_dx, ent_w, resp, lse, r2,
                                                                            kept, n, K, M, A, S, P, t_scale, dtheta, sigma2);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

long tvae_class_average_weighted_ws_floats(int E, int K, int C, int n) {
    if (!wavg_shape_ok(E, K, C, n)) return 0;
    return wavg_ws_need(E, K, C, n);
}

int tvae_class_average_weighted_chunk(int E, int K, int C, int n) { return wavg_shape_ok(E, K, C, n) ? WAVG_CHUNK : 0; }

int tvae_class_average_weighted(const float* Y, const int* img, const float* theta_e, const float* dx_e, const float* w,
                                const int* seg, float* avg, double* wsum, int* counts, float* ws, long ws_floats, int N, int E,
                                int C, int n, int K, float t_scale, tvae_stream_t stream) {
    if (!wavg_shape_ok(E, K, C, n) || !wavg_stack_ok(N, C, n)) return (int)hipErrorInvalidValue;
    if (!Y || !img || !theta_e || !dx_e || !w || !seg || !avg || !wsum || !counts || !ws) return (int)hipErrorInvalidValue;
    const long slots = wavg_slots(E, K), ints = wavg_ws_ints(E, K), need = wavg_ws_need(E, K, C, n);
    if (ws_floats < need || !aligned8(ws) || !aligned8(wsum)) return (int)hipErrorInvalidValue;
    const size_t f = sizeof(float), plane = (size_t)C * n * n * f, Es = (size_t)E;
    const Span in[] = {{Y, (size_t)N * plane}, {img, Es * f}, {theta_e, Es * f}, {dx_e, 2 * Es * f}, {w, Es * f},
                       {seg, ((size_t)K + 1) * f}};
    const Span out[] = {{avg, (size_t)K * plane}, {wsum, (size_t)K * sizeof(double)}, {counts, (size_t)K * f},
                        {ws, (size_t)need * f}};
    if (!outputs_clear(out, in)) return (int)hipErrorInvalidValue;
    int* clean = reinterpret_cast<int*>(ws);
    int* cnt = clean + (K + 1);
    double* wpart = reinterpret_cast<double*>(ws + ints);
    float* part = ws + ints + 2 * slots;
    const int tiles = wavg_tiles(n);
    hipStream_t s = tvae_cluster::S(stream);
    wavg_seg_kernel<<<1, WAVG_TILE, 0, s>>>(seg, clean, K, E);
    TVAE_CLUSTER_CHECK_LAUNCH();
    wavg_accum_kernel<<<(unsigned)(slots * C * tiles), WAVG_TILE, 0, s>>>(Y, img, theta_e, dx_e, w, clean, part, wpart, cnt, N,
                                                                         C, n, K, tiles, t_scale);
    TVAE_CLUSTER_CHECK_LAUNCH();
    wavg_reduce_kernel<<<(unsigned)((long)K * C * tiles), WAVG_TILE, 0, s>>>(part, wpart, cnt, clean, avg, wsum, counts, C, n,
                                                                            tiles);
    TVAE_CLUSTER_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
