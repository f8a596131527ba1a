/* C ABI of libtvae_cluster.so: batched Lloyd k-means on the GPU (gfx950), the hot path of clustering_*.py.
 *
 * Same conventions as tvae_hip.h: raw device pointers and sizes, the stream as void*, `int` return = hipError_t.  The
 * entry points never allocate, free or synchronise and keep no process-wide state; the workspace is the caller's,
 * sized by the pure host query tvae_kmeans_ws_floats.
 *
 * Layout: points FEATURE-major, Xt[d][ldx] (ldx >= N; lanes run along the contiguous point index; ldx % 4 == 0 and a
 * 16-byte aligned Xt take the vector loads).  Centroids C[R][k][d]: R restarts advance in ONE launch; a restart r with
 * done[r] != 0 is skipped entirely (nothing of it is read or written).
 *
 * Arithmetic: distances in the direct form sum_j (x_j - c_j)^2, fp32, ascending j (error relative to the distance
 * itself, two equal centroids give bit-identical distances); ties go to the lowest cluster index.  No float atomics:
 * every output is a pure function of the inputs, bitwise reproducible, and a restart's results do not depend on R or
 * on the other restarts of the launch (the split of the points into G groups depends on N, d, k only).
 *
 * Supported: 1 <= d <= 256, 1 <= k <= 1024, k <= N, 1 <= R <= TVAE_KMEANS_MAX_RESTARTS (65535: the restarts are the y
 * dimension of the launch grid), R * N < 2^31; anything else returns hipErrorInvalidValue (1) and writes nothing.
 */
#ifndef TVAE_CLUSTER_H
#define TVAE_CLUSTER_H
#ifdef __cplusplus
extern "C" {
#endif

typedef void* tvae_stream_t;

#define TVAE_KMEANS_MAX_RESTARTS 65535

int tvae_cluster_abi_version(void);          /* == 1 */

/* floats of workspace for one assign / update pair: per restart G x (k*d sums, k counts, 1 changed count, 1 sum of
 * mind2), G = tvae_kmeans_groups(N, d, k).  0 for unsupported arguments. */
long tvae_kmeans_ws_floats(int N, int d, int k, int R);
/* number of point groups per restart (a pure function of N, d, k; never of R) */
int tvae_kmeans_groups(int N, int d, int k);

/* labels[R][N] (in: previous labels, out: new), mind2[R][N], changed[R] = number of points whose label differs from
 * the one that was in `labels`; ws: per (restart, group) partial sums [G][k][d], counts [G][k] and scalars. */
int tvae_kmeans_assign(const float* Xt, long ldx, const float* C, const int* done, int* labels, float* mind2,
                       int* changed, float* ws, long ws_floats, int N, int d, int k, int R, tvae_stream_t stream);

/* reduces the partials of the preceding assign in a fixed order: C[r][c] <- mean of its points (a cluster without
 * points keeps its centroid bit for bit), inertia[r] = sum mind2, shift[r] = sum ||C_new - C_old||^2 */
int tvae_kmeans_update(const float* ws, long ws_floats, const int* done, float* C, float* inertia, float* shift,
                       int N, int d, int k, int R, tvae_stream_t stream);

/* the D^2 step of k-means++: D[r][n] = min(D[r][n], ||x_n - cnew[r]||^2), cnew[R][d] */
int tvae_kmeans_mindist(const float* Xt, long ldx, const float* cnew, float* D, int N, int d, int R,
                        tvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TVAE_CLUSTER_H */
