/* C ABI of libtvae_cluster.so: batched Lloyd k-means, Ward linkage, exact t-SNE, aligned class averages and their half
 * sets, variance maps and ring correlation on the GPU (gfx950), the hot paths of clustering_*.py, class_averages.py and
 * class_resolution.py.
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

/* Still 1: the Ward, t-SNE, alignment, pose-refinement, reassignment, pose-polish, class-statistics, preprocessing, CTF,
 * eigenimage and maximum-likelihood entry points below were
 * ADDED, no existing prototype or meaning changed. */
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

/* ---- Ward agglomerative clustering without an N x N matrix ----------------------------------------------------------
 *
 * State of a round: M live clusters in slots 0 .. M-1, centroids FEATURE-major Ct[d][ld] (ld >= M; ld % 4 == 0 and a
 * 16-byte aligned base take the vector loads, anything else a scalar instance with the same arithmetic), sizes cnt[M]
 * as fp32 (exact up to 2^24), node ids id[M] and hmax[M] (fp64), the recorded height of the merge that made the slot (0
 * for a leaf).
 *
 * Arithmetic: w(i,j) = (cnt_i * cnt_j) / (cnt_i + cnt_j) * sum_f (c_if - c_jf)^2, every operation rounded to fp32 on its
 * own, the sum an FMA chain in ascending f.  It is bitwise symmetric, w(i,j) == w(j,i).  Ties go to the lowest j
 * (strict < in ascending j, also where the partial minima of column ranges are combined; the split into ranges
 * depends on (M, d) only).  Symmetry and the tie rule make the lexicographically least pair at the global minimum
 * reciprocal, so a round over finite inputs merges at least one pair.  No float atomics; outputs are bitwise
 * reproducible.
 *
 * Supported: 2 <= M <= 2^24, 1 <= d <= 256, M <= N <= 2^24; anything else returns hipErrorInvalidValue (1) and writes
 * nothing. */

/* floats of workspace of tvae_ward_nn: the partial (minimum, argmin) of tvae_ward_nn_splits(M, d) column ranges per
 * row.  0 for unsupported arguments. */
long tvae_ward_nn_ws_floats(int M, int d);
int tvae_ward_nn_splits(int M, int d);
/* ints of workspace of tvae_ward_merge (compacted position and pair rank per slot).  0 for unsupported arguments. */
long tvae_ward_merge_ws_ints(int M, int d);

/* nn[i] = argmin over j != i of w(i,j) and nd[i] = that minimum.  A row whose every w is +inf or NaN gets the lowest
 * j != i and nd = +inf. */
int tvae_ward_nn(const float* Ct, long ldc, const float* cnt, int* nn, float* nd, float* ws, long ws_floats, int M,
                 int d, tvae_stream_t stream);

/* One round of merges.  The centroids are kept in fp64, C[d][ld] (same layout); Ct_out receives their fp32 rounding,
 * which is what tvae_ward_nn searches.  Every pair i < j with nn[i] == j and nn[j] == i is merged; its rank r counts
 * such pairs by ascending i.  Record base + r: rec_ids[base + r] = (id_i then id_j) and rec_hs[base + r] = (height then
 * cnt_i + cnt_j) with height = max(sqrt(2 w64(i j)) and hmax_i and hmax_j) where w64 is the formula above in fp64 on
 * the fp64 centroids: heights never decrease from child to parent.  The merged cluster has the centroid
 * (cnt_i c_i + cnt_j c_j) / (cnt_i + cnt_j) in fp64 and the temporary id N + base + r and takes the place of slot i.
 * Survivors go to the *_out arrays compactly in ascending old slot order (ld_out >= M) and their number to *m_out.
 * cap = records that rec_ids / rec_hs hold; base + M / 2 <= cap is required.  The *_out arrays must not overlap the
 * inputs. */
int tvae_ward_merge(const double* C_in, long ld_in, const float* cnt_in, const int* id_in, const double* hmax_in,
                    const int* nn, double* C_out, float* Ct_out, long ld_out, float* cnt_out, int* id_out,
                    double* hmax_out, int* rec_ids, double* rec_hs, int* m_out, int* ws, long ws_ints, int M, int d,
                    int N, int base, int cap, tvae_stream_t stream);

/* ---- t-SNE of the latents: sparse input similarities from brute-force kNN, exact all-pairs repulsion -----------------
 *
 * Points FEATURE-major as above, Xt[d][ldx]; the 2-D embedding, its gains, its last update and the repulsion sums share
 * one layout, [2][ldy] (ldy >= N; ldy % 4 == 0 and a 16-byte aligned base take the vector loads, anything else a scalar
 * instance with the same arithmetic).  P is CSR: rowptr[N + 1], col[nnz], val[nnz] (fp32); entries outside [0, nnz) and
 * columns outside [0, N) are skipped, never dereferenced.  q_ij = 1 / (1 + |y_i - y_j|^2) in fp32 (reciprocal
 * instruction, 1 ulp); j == i is excluded BY INDEX, so a duplicate of point i is an ordinary neighbour at distance 0.
 * No float atomics: every output is a pure function of the inputs, bitwise reproducible; the split of the columns into
 * ranges depends on N only.  Sums that cross rows (Z, the KL divergence, |grad|^2) are fp64 in a fixed order.
 *
 * Supported: 2 <= N <= 2^24; tvae_knn also 1 <= d <= 256 and 1 <= K <= 256 with K < N; 1 <= nnz < 2^31; anything else
 * returns hipErrorInvalidValue (1) and writes nothing. */

/* workgroups of 256 rows: the number of |grad|^2 partials of tvae_tsne_step and of fp64 workspace words of
 * tvae_tsne_kl.  0 for unsupported arguments. */
int tvae_tsne_groups(int N);
/* floats of workspace of tvae_tsne_repulsion (8-byte aligned): per-workgroup fp64 partials of Z and per column range
 * three fp32 partials per row.  0 for unsupported arguments. */
long tvae_tsne_repulsion_ws_floats(int N);

/* idx[N][K] and d2[N][K]: the K nearest neighbours of every point other than itself and their squared distances in the
 * direct form sum_f (x_f - c_f)^2 (fp32 FMA chain in ascending f), each row sorted ascending by (d2 then index).  A
 * non-finite distance is never selected (a row without K finite ones keeps idx = -1 and d2 = +inf at its end). */
int tvae_knn(const float* Xt, long ldx, int* idx, float* d2, int N, int d, int K, tvae_stream_t stream);

/* rep[c][i] = sum over j != i of q_ij^2 (y_ci - y_cj) (fp32 row sums) and Z[0] = sum over i != j of q_ij (fp32 per row
 * and column range, everything above that in fp64). */
int tvae_tsne_repulsion(const float* Yt, long ldy, float* rep, double* Z, float* ws, long ws_floats, int N,
                        tvae_stream_t stream);

/* One gradient-descent step.  grad_i = 4 (exaggeration * sum_e val_e q_ie (y_i - y_col(e)) - rep_i / Z); sklearn's rule:
 * gains += 0.2 where update * grad < 0 and *= 0.8 elsewhere with floor 0.01; update = momentum * update - learning_rate *
 * gains * grad; Yt_out = Yt + update.  gains and update are updated in place (a row only touches its own), the
 * embedding is NOT: Yt_out must be a second buffer, other rows still read the old Yt.  grad (may be NULL) receives the
 * gradient; gnorm2[tvae_tsne_groups(N)] the fp64 sum of |grad_i|^2 of every 256 rows. */
int tvae_tsne_step(const int* rowptr, const int* col, const float* val, long nnz, const float* Yt, const float* rep,
                   const double* Z, float* gains, float* update, float* Yt_out, float* grad, double* gnorm2, long ldy,
                   int N, float exaggeration, float momentum, float learning_rate, tvae_stream_t stream);

/* kl[0] = sum over the CSR entries of val ln(max(val, eps) / max(q / Z, eps)) with eps = 2^-52, in fp64 throughout;
 * ws holds tvae_tsne_groups(N) fp64 words. */
int tvae_tsne_kl(const int* rowptr, const int* col, const float* val, long nnz, const float* Yt, long ldy,
                 const double* Z, double* kl, double* ws, long ws_doubles, int N, tvae_stream_t stream);

/* ---- Aligned images and aligned 2-D class averages of a clustered stack ------------------------------------------------
 *
 * Y[N][C][n][n] (square images, all channels of an image share one pose), theta[N] and dx[N][2] as the encoder predicts
 * them, t_scale the factor between dx and coordinate units (1 where the translation was inferred by attention, 0.1 for
 * the unimodal encoder, the reference's dx_scale).  The model's convention: coordinates linspace(-1, 1, n) along columns
 * and linspace(1, -1, n) along rows, a pixel at x shows canonical content at u = (x - t dx) R(theta).  The aligned image
 * A_i at the canonical grid point u = (u0, u1) therefore reads image i at
 *     x = (u0 c + u1 s + t dx0,  -u0 s + u1 c + t dx1),  c = cos theta_i, s = sin theta_i (accurate cosf / sinf),
 *     col = (x0 + 1) (n - 1) / 2,  row = (1 - x1) (n - 1) / 2,
 * bilinear over the taps floor and floor + 1 per axis.  A tap outside [0, n - 1] is 0 (zero border: the sample is a
 * continuous function of the position); a position that is not inside (-1, n) on both axes gives exactly 0, which
 * covers NaN, +-inf and huge poses (the range is tested before any float -> int conversion).
 *
 * Class averages: order[N] holds image indices grouped by class, seg[K + 1] the class boundaries in `order` (both device
 * pointers; class k = order[seg[k] .. seg[k + 1])), avg[k] = (sum of A_i over the members) / (number of members).
 * Entries of `order` outside [0, N) are skipped, never dereferenced, and do not count; a class without members gives
 * zeros.  seg is never read on the host; on the device it is replaced by min(max(0, seg[0], ..., seg[k]), N), which
 * leaves a monotone seg within [0, N] as it is and makes any other one monotone: nothing is followed out of bounds.
 * The aligned stack is never written: a class is cut into chunks of tvae_class_average_chunk consecutive members, counted
 * from the class's own first member; the fp32 sum of a chunk in ascending position goes to the workspace and a second
 * launch adds the chunks of a class in ascending order and divides.
 * No float atomics: every output is a pure function of the inputs, bitwise reproducible.  The split of a class into chunks
 * depends on (seg, N, K, C, n) only, and avg[k] only on class k's ordered member list and those members' images and
 * poses: not on the other classes, not on K.
 *
 * Supported: 1 <= N <= 2^24, 1 <= C <= 1024, 2 <= n <= 1024, 1 <= K <= 65535, fewer than 2^31 workgroups of 256 pixels
 * (N C ceil(n n / 256), and (N / chunk + K) C ceil(n n / 256) for the averages); anything else returns
 * hipErrorInvalidValue (1) and writes nothing. */

/* floats of workspace of tvae_class_average: the cleaned seg and one member count per chunk slot (int32 words) and the
 * partial sums of N / chunk + K slots.  0 for unsupported arguments. */
long tvae_class_average_ws_floats(int N, int K, int C, int n);
/* members per chunk (a constant of the build, 32).  0 for unsupported arguments. */
int tvae_class_average_chunk(int N, int K, int C, int n);

/* out[N][C][n][n] = A_i; out must not be Y. */
int tvae_align_stack(const float* Y, const float* theta, const float* dx, float* out, int N, int C, int n,
                     float t_scale, tvae_stream_t stream);

/* avg[K][C][n][n]; ws holds tvae_class_average_ws_floats(N, K, C, n) floats. */
int tvae_class_average(const float* Y, const float* theta, const float* dx, const int* order, const int* seg, float* avg,
                       float* ws, long ws_floats, int N, int C, int n, int K, float t_scale, tvae_stream_t stream);

/* ---- Pose refinement against the class averages --------------------------------------------------------------------------
 *
 * The inverse of the map above: instead of resampling the image into the canonical frame, the class average of the image's
 * class is rendered into the image's frame at NA = 2A + 1 angles, and compared with the image at NS x NS whole-pixel shifts,
 * NS = 2S + 1.  Y, theta, dx and t_scale (> 0) as in tvae_align_stack; cls[N] (int32) the class of every image;
 * ref[K][C][n][n] the class averages in the canonical frame; dtheta the angle step in radians (finite); mask_radius and
 * mask_edge in pixels.
 *
 * Template.  For image i with k = cls[i] and the angle index a = -A .. A: theta_a = theta[i] + (float)a * dtheta (the product
 * and the sum each rounded to fp32), c = cos theta_a, s = sin theta_a (accurate cosf / sinf).  For every pixel (r, q) of the
 * EXTENDED grid, r and q = -S .. n - 1 + S:
 *     x0 = 2 q / (n - 1) - 1,  x1 = 1 - 2 r / (n - 1),  v = x - t dx[i],
 *     u0 = v0 c - v1 s,  u1 = v0 s + v1 c,  col = (u0 + 1) (n - 1) / 2,  row = (1 - u1) (n - 1) / 2,
 *     T_a[ch][r][q] = m(u) * (the bilinear sample of ref[k][ch] at (row, col)),
 * with the sampling rules of the section above: taps floor and floor + 1, a tap outside [0, n - 1] is 0, and a position that
 * is not inside (-1, n) on both axes gives exactly 0, mask or no mask (tested before any float -> int conversion: NaN, +-inf
 * and huge poses give a template of zeros).  m is the mask of tvae_class_frc (below) at d = sqrt(u0^2 + u1^2) (n - 1) / 2
 * pixels from the canonical centre, evaluated in fp64 from the fp32 u: 1 for d <= mask_radius, the raised cosine over
 * mask_edge, 0 beyond; mask_radius <= 0 means no mask; a non-finite radius or edge and a negative edge are rejected.
 *
 * Candidates.  The candidate (a, sy, sx), sy and sx = -S .. S, predicts P(r, q) = T_a[r - sy][q - sx] on the frame
 * r, q = 0 .. n - 1:
 *     num = sum P Y,  pp = sum P^2  (over channels and pixels),   yy = sum Y^2 over the whole frame,
 *     score = num / sqrt(pp yy) in fp64 from the three fp32 sums, rounded to fp32 once; exactly 0 where pp or yy is 0:
 * the cosine between the image and what the model predicts at that pose.  The candidate is the pose
 *     theta' = theta_a,   dx' = dx + (2 sx / (n - 1), -2 sy / (n - 1)) / t_scale
 * (fp32: (float)(2 sx) / (float)(n - 1), then / t_scale, then the sum, each correctly rounded).  A part of the pose whose index
 * (a, sx or sy) is 0 is copied bit for bit.
 *
 * Selection.  The best candidate starts as the centre (0, 0, 0); the candidates are visited in ascending (a, sy, sx) and one
 * replaces the best only if its score is finite and strictly greater.  An image whose pose cannot be improved keeps theta and
 * dx bit for bit, and the refined score is never below the centre score.  A centre score that is not finite counts as -inf
 * (and is reported as -inf in score[i][0]); if no candidate is finite the pose is unchanged and both scores are 0.
 * An image with cls outside [0, K) keeps its pose bit for bit and gets the scores (0, 0), best (0, 0, 0) and zeros in its rows
 * of the tables; nothing of ref is read for it.
 *
 * Arithmetic: fp32 products and sums (FMA chains) in a fixed order, no atomics.  num of a candidate: the rows of the frame are
 * dealt to G groups by r mod G, where G = ceil(n / ceil(n / (256 div NS))); a group adds channel after channel, within a
 * channel its rows in ascending r and along a row the pixels in ascending q, one chain; the G sums are then added in ascending
 * group.  pp: R2[re][sx] = the sum of T^2 over the n columns of the window in row re of the extended template, one chain in
 * ascending q that runs on through the channels; pp = the sum of R2 over the window's n rows in ascending r.  yy: thread t of
 * 256 adds the pixels p = t, t + 256, ... of every channel in turn in one chain, then a binary tree over the 256 sums (t and
 * t + 128, then t and t + 64, ...).  Every output of image i is a pure function of image i, its pose and ref[cls[i]]: not of
 * N, K or the other images; every output is bitwise reproducible.
 *
 * Supported: 1 <= N <= 2^24, 1 <= C <= 16, 2 <= n <= 128 (one image plane and one extended template fit the 160 KB of LDS),
 * 1 <= K <= 65535, 0 <= A <= 32, 0 <= S <= 8, t_scale finite and > 0, dtheta finite; num and pp both NULL or both not; no
 * output (the workspace is one) may overlap an input.  Anything else returns hipErrorInvalidValue (1) and writes nothing, and
 * the query returns 0. */

/* floats of workspace of tvae_pose_refine: the tables num and pp [N][NA][NS][NS] and yy [N] (used where the caller passes
 * NULL for them).  0 for unsupported arguments. */
long tvae_pose_refine_ws_floats(int N, int C, int n, int A, int S);

/* theta_out[N], dx_out[N][2], score[N][2] = (centre, best), best[N][3] = (a, sy, sx) (int32); num and pp [N][NA][NS][NS] or
 * both NULL, yy[N] or NULL: the raw sums, for tests */
int tvae_pose_refine(const float* Y, const float* theta, const float* dx, const int* cls, const float* ref,
                     float* theta_out, float* dx_out, float* score, int* best, float* num, float* pp, float* yy, float* ws,
                     long ws_floats, int N, int C, int n, int K, int A, int S, float t_scale, float dtheta,
                     float mask_radius, float mask_edge, tvae_stream_t stream);

/* ---- Reassignment against the class averages -----------------------------------------------------------------------------
 *
 * The other half of the averaging loop: the pose search of the section above against M candidate classes per image instead
 * of one, and the choice among them (multi-reference alignment).  All classes share the decoder's canonical frame, so the
 * predicted pose of an image is close to right for every class and the small neighbourhood of tvae_pose_refine is enough.
 * Y, theta, dx, ref[K][C][n][n], t_scale, A, S, dtheta, mask_radius and mask_edge as for tvae_pose_refine;
 * cand[N][M] (int32), 1 <= M <= TVAE_CLASSIFY_MAX_CANDIDATES: the candidate classes of every image, slot 0 by convention
 * its current class.  A slot whose value is outside [0, K) is skipped: nothing of ref is read for it, its rows of the tables
 * are zeros and its scores are (0, 0).  Duplicates are allowed and computed as given.
 *
 * Per slot.  For slot m with k = cand[i][m] the sums num, pp [N][M][NA][NS][NS] and yy [N] are bit for bit what
 * tvae_pose_refine produces for that image with cls[i] = k: the templates, the chains and their order, the score in fp64
 * from the three fp32 sums and the selection rule with its centre priority are those of the section above, and so are the
 * slot's score[i][m] = (centre, best) and its best candidate (a, sy, sx).  yy is formed once per image; it is 0 for an
 * image with no valid slot.
 *
 * Across slots.  The valid slots compete with the best score they report.  They are visited in ascending m: the first valid
 * slot is the start, and a later slot replaces it only if its best score is strictly greater.  Ties therefore stay with the
 * lowest slot -- the incumbent when slot 0 is valid.  A slot with no finite candidate reports 0 and competes with that 0.
 *
 * Outputs.  With m* the winning slot: cls_out[i] = cand[i][m*], best[i] = (m*, a, sy, sx) of that slot's best candidate, and
 * theta_out, dx_out by the pose update of tvae_pose_refine applied to it (an index that is 0 copies its part of the pose bit
 * for bit).  An image with no valid slot keeps its pose bit for bit and gets cls_out = cand[i][0] unchanged, best = 0 and
 * zero scores.  Every output of image i is a pure function of image i, its pose, its row of candidates and the references
 * that row names: not of N, K or the other images.  No atomics; every output is bitwise reproducible.
 *
 * Supported: the range of tvae_pose_refine and 1 <= M <= 64; num and pp both NULL or both not, yy may be NULL (the workspace
 * holds what is not given); no output (the workspace is one) may overlap an input.  Anything else returns
 * hipErrorInvalidValue (1) and writes nothing, and the query returns 0. */

#define TVAE_CLASSIFY_MAX_CANDIDATES 64

/* floats of workspace of tvae_pose_classify: N (2 M NA NS^2 + 1), the tables num and pp [N][M][NA][NS][NS] and yy [N] (used
 * where the caller passes NULL for them).  0 for unsupported arguments. */
long tvae_pose_classify_ws_floats(int N, int M, int C, int n, int A, int S);

/* cls_out[N] (int32), best[N][4] = (m*, a, sy, sx) (int32), theta_out[N], dx_out[N][2], score[N][M][2] = (centre, best) of
 * every slot; num and pp [N][M][NA][NS][NS] or both NULL, yy[N] or NULL: the raw sums, for tests */
int tvae_pose_classify(const float* Y, const float* theta, const float* dx, const int* cand, const float* ref, int* cls_out,
                       int* best, float* theta_out, float* dx_out, float* score, float* num, float* pp, float* yy, float* ws,
                       long ws_floats, int N, int C, int n, int K, int M, int A, int S, float t_scale, float dtheta,
                       float mask_radius, float mask_edge, tvae_stream_t stream);

/* ---- Sub-pixel pose polish against the class averages: Gauss-Newton on the cosine score ---------------------------------
 *
 * The grid searches above leave a translation error of up to half a pixel per axis.  The polish is the continuous local
 * step after them: Levenberg-Marquardt on || Y - alpha P(theta, t dx) ||^2, whose minimum over alpha is the maximum of the
 * cosine score.  One evaluation (tvae_pose_moments) renders ONE template per image with its derivatives and reduces them
 * to 15 sums; the bookkeeping (tvae_pose_polish_step) is a thread per image in fp64 on those sums, so the host loop is
 * launches only:  moments(start) -> step(first = 1) -> [moments(trial) -> step(first = 0)] x iterations.
 * Y, theta, dx, cls, ref, t_scale, mask_radius and mask_edge as for tvae_pose_refine.
 *
 * tvae_pose_moments.  For image i with k = cls[i], at every pixel (r, q) of the frame: the position (u0, u1), (col, row) of
 * tvae_pose_refine's template at A = 0, S = 0 -- the same fp32 arithmetic, operation for operation -- and with it the same
 * bilinear sample B of ref[k][ch] (zero border; exact 0 out of frame) and the same mask m(u).  With the taps a00, a01 (row
 * floor), a10, a11 (row floor + 1) of that sample, already zeroed by the border rule, and its weights wc, wr:
 *     top = a00 + wc (a01 - a00),  bot = a10 + wc (a11 - a10),  B = top + wr (bot - top),
 *     Bc = (1 - wr) (a01 - a00) + wr (a11 - a10),   Br = bot - top:
 * the derivatives of the SAME cell that produced the sample, exact 0 where the sample is the out-of-frame 0.  With
 * h = (n - 1) / 2 the basis functions on the frame are
 *     P = m B,   G0 = m h Bc  (dP / du0),   G1 = -m h Br  (dP / du1),   Dtheta = -u1 G0 + u0 G1   (0 out of frame).
 * The mask is held CONSTANT under the derivative, deliberately: the direction is quasi-Newton, acceptance uses the exact
 * score, and a hard edge has no derivative anyway.
 * mom[i][0 .. 14], sums over channels and pixels:  PP, P Dtheta, P G0, P G1, Dtheta Dtheta, Dtheta G0, Dtheta G1, G0 G0, G0 G1,
 * G1 G1;  P Y, Dtheta Y, G0 Y, G1 Y;  Y Y.  mom[i][0] and mom[i][10] are pp and num of the centre candidate of tvae_pose_refine
 * (A = 0, S = 0) up to the order of addition, and mom[i][14] is its yy bit for bit.
 * Order of addition, that of yy in tvae_pose_refine: thread t of 256 takes the pixels t, t + 256, ... of channel 0, then of
 * channel 1, ..., one fmaf chain per sum; then a binary tree over the 256 sums (t and t + 128, then t and t + 64, ...).  No
 * atomics, bitwise reproducible; row i is a function of image i, its pose and ref[cls[i]] only, not of N or K.
 * An image with cls outside [0, K) gets 15 exact zeros and nothing of ref is read for it; a pose that puts every sample out
 * of frame (NaN, +-inf, huge) gives zeros in the first 14 sums and the true yy.
 * Supported: 1 <= N <= 2^24, 1 <= C <= 16, 2 <= n <= 128, 1 <= K <= 65535, t_scale finite and > 0, the mask rules of
 * tvae_pose_refine; mom may not overlap an input.  Anything else returns hipErrorInvalidValue (1) and writes nothing.
 *
 * tvae_pose_polish_step.  State per image, all in the caller's arrays: the start pose theta0, dx0 (input: the centre of the
 * trust region), the current pose theta_out, dx_out with its moments mom_cur and score[i] = (start, current), the damping
 * lambda (fp64), the trial pose theta_try, dx_try, whose moments the caller puts into mom_try before every call, the number
 * of accepted steps and the flag `ended`.  Every operation below is fp64, rounded on its own, in the order written.
 *   first != 0 (mom_try holds the moments of the start pose): current <- start, mom_cur <- mom_try, both scores <- its score,
 *     lambda <- 1e-3, steps <- 0.  An image with cls outside [0, K) or a start score that is not finite gets the scores
 *     (0, 0), trial = current = start bit for bit and ended = 1.
 *   first == 0: an ended image is left alone entirely.  Otherwise the trial is accepted iff its score is finite and
 *     STRICTLY greater than the current one: trial -> current (pose, moments, score[i][1]), lambda <- lambda / 4, steps + 1;
 *     if not, lambda <- 8 lambda.
 *   Score: PY / sqrt(PP YY) in fp64 from the fp32 sums, exactly 0 where PP or YY is 0 (tvae_pose_refine's rule), compared
 *     in fp64 -- near the optimum two poses differ by less than an fp32 step of the cosine -- and rounded to fp32 only
 *     where it is stored in `score`.  The current score is formed again from mom_cur at every call.
 *   Next trial, from the moments of the current pose.  c and s: the cosine and sine of the fp32 theta evaluated in fp64 and
 *     rounded to fp32 once (the correctly rounded cosf / sinf, so that a host restatement has the same bits), as doubles;
 *     (Dtx, Dty) = (-c G0 - s G1, s G0 - c G1), the derivatives along t dx; their sums:
 *       P Dtx = -(c PG0) - s PG1,  P Dty = s PG0 - c PG1,  and the same for Dtheta and for Y in the place of P;
 *       DtxDtx = (c c) G0G0 + (2 (c s)) G0G1 + (s s) G1G1,   DtyDty = (s s) G0G0 - (2 (c s)) G0G1 + (c c) G1G1,
 *       DtxDty = ((c c - s s) G0G1 - (c s) G0G0) + (c s) G1G1      (sums left to right).
 *     alpha = PY / PP.  Unknowns x = (dtheta, dtx, dty, dalpha) of || Y - alpha P ||^2, J = [alpha Dtheta, alpha Dtx,
 *     alpha Dty, P]:  M = J^T J with M[a][b] = (alpha alpha) <Da Db> for a, b < 3, M[a][3] = alpha <P Da>, M[3][3] = PP;
 *     rhs[a] = alpha (<Da Y> - alpha <P Da>), rhs[3] = PY - alpha PP; then M[a][a] <- M[a][a] + lambda M[a][a].
 *     Gaussian elimination with partial pivoting: for column k = 0 .. 3 the pivot is the first row r >= k of the largest
 *     |M[r][k]| (rows swapped); for r > k: f = M[r][k] / M[k][k], M[r][j] <- M[r][j] - f M[k][j] for j > k,
 *     rhs[r] <- rhs[r] - f rhs[k]; back substitution x[i] = (rhs[i] - M[i][i+1] x[i+1] - ... ) / M[i][i], subtracted in
 *     ascending j.  PP = 0, YY = 0, a zero or non-finite pivot or a non-finite solution mean "no step".
 *     New pose: theta + dtheta, dx + (dtx, dty) / t_scale in fp64, clamped per component to the trust region
 *     [centre - radius, centre + radius] (centre the start pose; radius max_angle for theta and
 *     ((max_shift * 2) / (n - 1)) / t_scale for dx), rounded to fp32 once; a rounded value outside the region is moved one
 *     fp32 step towards the centre.  A trial that is not finite is "no step".
 *   A trial equal to the current pose bit for bit ("no step" among it) ends the image: ended = 1.
 * After the last call theta_out, dx_out, score and steps are the result; score[i][1] >= score[i][0] always.
 * Supported: 1 <= N <= 2^24, 2 <= n <= 128, 1 <= K <= 65535, t_scale finite and > 0, max_shift (pixels) and max_angle
 * (radians) finite and >= 0; lambda 8-byte aligned; none of the nine state arrays (theta_try .. ended) may overlap another or
 * an input.  Anything else returns hipErrorInvalidValue (1) and writes nothing. */

/* mom[N][15] */
int tvae_pose_moments(const float* Y, const float* theta, const float* dx, const int* cls, const float* ref, float* mom, int N,
                      int C, int n, int K, float t_scale, float mask_radius, float mask_edge, tvae_stream_t stream);

/* cls[N] (int32), theta0[N], dx0[N][2], mom_try[N][15]: inputs.  theta_try[N], dx_try[N][2], theta_out[N], dx_out[N][2],
 * mom_cur[N][15], score[N][2], lambda[N] (fp64), steps[N], ended[N] (int32): the state, written by the first call */
int tvae_pose_polish_step(const int* cls, const float* theta0, const float* dx0, const float* mom_try, float* theta_try,
                          float* dx_try, float* theta_out, float* dx_out, float* mom_cur, float* score, double* lambda,
                          int* steps, int* ended, int N, int n, int K, int first, float t_scale, float max_shift,
                          float max_angle, tvae_stream_t stream);

/* ---- Quality of the class averages: half sets, variance maps and the Fourier ring correlation ---------------------------
 *
 * tvae_class_halves is tvae_class_average with three accumulators per pixel, in the same single pass over the stack: the
 * pose convention, the sampling, the zero border and the out-of-frame rule are those of the section above, `order`
 * entries outside [0, N) are skipped, seg is cleaned on the device in the same way, and the chunks and slots are the same
 * (tvae_class_average_chunk members counted from the class's own first position).
 *
 * Halves: position q of a member counts from the class's first position in `order`; a skipped entry keeps its position.
 * Half 0 takes the even q, half 1 the odd q (a chunk starts at an even position, so the parity within the chunk is the
 * half).  Per pixel and chunk three fp32 sums in ascending position, S0 over the even members, S1 over the odd ones and
 * Q = sum A^2 over all of them (each sample is taken once), and the two member counts n0, n1.  A second launch adds the
 * chunks of a class in ascending order in fp64 and writes, each rounded to fp32 once,
 *     half[h] = S_h / n_h (zeros where n_h = 0),   avg = (S0 + S1) / (n0 + n1) (zeros for an empty class),
 *     var = max(0, (Q - (S0 + S1)^2 / m) / (m - 1)) with m = n0 + n1, and 0 for m < 2,
 * and counts[k] = (n0, n1).
 * avg agrees with tvae_class_average to rounding, NOT bit for bit: the order of addition differs (two interleaved fp32
 * sums per chunk and fp64 above them, against one fp32 sum throughout).
 * The variance is the sum-of-squares form: its error is relative to Q / m, not to the variance itself.  That is fine for
 * normalised particles (mean near 0, spread near 1) and poor for images whose mean dwarfs their spread.
 * No float atomics: every output is a pure function of the inputs, bitwise reproducible, and every output of class k
 * depends on class k's ordered member list and those members' images and poses only: not on the other classes, not on K.
 *
 * Supported: the range of tvae_class_average with the slot count tripled where it bounds the grid,
 * 3 (N / chunk + K) C ceil(n n / 256) < 2^31; anything else returns hipErrorInvalidValue (1) and writes nothing.
 *
 * tvae_class_frc: the Fourier ring correlation of P pairs of planes a[p], b[p] (n x n); planes are independent, a NaN in
 * a plane stays in that plane's results.
 * Mask: with d the distance of pixel (i, j) from ((n - 1) / 2, (n - 1) / 2), m = 1 for d <= mask_radius,
 * m = (1 + cos(pi (d - mask_radius) / mask_edge)) / 2 for mask_radius < d < mask_radius + mask_edge and 0 beyond;
 * mask_radius <= 0 means no mask, mask_edge = 0 a hard edge; a non-finite radius or edge and a negative edge are
 * rejected.
 * Transform: F(ky, kx) = sum_ij a[i][j] m(i, j) exp(-2 pi i (ky i + kx j) / n), ky and kx the signed frequencies in the
 * order of numpy's fftfreq; a direct DFT in two stages (rows to the half spectrum kx = 0 .. n / 2, then columns) with fp32
 * products and sums and a table of the n twiddles whose argument is reduced exactly, (i k) mod n in integers, each entry
 * within an ulp.
 * Rings: the ring of (ky, kx) is the integer r with r - 1/2 <= sqrt(ky^2 + kx^2) < r + 1/2, decided in exact integer
 * arithmetic as (2r - 1)^2 <= 4 (ky^2 + kx^2) < (2r + 1)^2 for r >= 1 and 4 (ky^2 + kx^2) < 1 for r = 0 (round half up,
 * no float comparison).  Rings 0 .. n / 2 (integer division) are kept, the corners beyond are dropped.
 *     sums[p][r] = (sum Re(Fa conj Fb), sum |Fa|^2, sum |Fb|^2) over the ring of the FULL plane,
 * accumulated in fp64 in a fixed order (ascending ky index, then ascending kx, over the half spectrum with its Hermitian
 * weights; the three products of a coefficient are formed in fp64 and rounded to fp32 once), no atomics;
 *     frc[p][r] = sums0 / sqrt(sums1 sums2) in fp64, rounded to fp32; exactly 0 where either power is 0.
 *
 * Supported: 2 <= n <= 1024, 1 <= P <= TVAE_FRC_MAX_PLANES (65535: the planes are the y dimension of the launch grids), ws
 * 8-byte aligned; anything else returns hipErrorInvalidValue (1) and writes nothing, and the queries return 0. */

#define TVAE_FRC_MAX_PLANES 65535

/* floats of workspace of tvae_class_halves: the cleaned seg and two member counts per chunk slot (int32 words, padded to
 * a multiple of 4) and three partial sums per pixel of N / chunk + K slots.  0 for unsupported arguments. */
long tvae_class_halves_ws_floats(int N, int K, int C, int n);

/* avg[K][C][n][n], half[2][K][C][n][n], var[K][C][n][n], counts[K][2] (int32) */
int tvae_class_halves(const float* Y, const float* theta, const float* dx, const int* order, const int* seg, float* avg,
                      float* half, float* var, int* counts, float* ws, long ws_floats, int N, int C, int n, int K,
                      float t_scale, tvae_stream_t stream);

/* number of rings, n / 2 + 1 (integer division).  0 for unsupported n. */
int tvae_frc_rings(int n);
/* floats of workspace of tvae_class_frc: per plane the half spectra of the rows of a and b (4 n R) and the three products
 * of every coefficient (3 n R), R = tvae_frc_rings(n).  0 for unsupported arguments. */
long tvae_class_frc_ws_floats(int P, int n);

/* a[P][n][n], b[P][n][n] -> frc[P][R] (fp32), sums[P][R][3] (fp64), R = tvae_frc_rings(n) */
int tvae_class_frc(const float* a, const float* b, float* frc, double* sums, float* ws, long ws_floats, int P, int n,
                   float mask_radius, float mask_edge, tvae_stream_t stream);

/* ---- Particle preprocessing: Fourier downsample (with the crop as its window) and background-ring normalisation ----------
 *
 * Downsample.  A window of M x N pixels of a frame X[B][H][W] is given by (r0, c0, M, N); it goes to m x n, 1 <= m <= M and
 * 1 <= n <= N.  With F(ky, kx) = sum_ab x[a][b] exp(-2 pi i (ky a / M + kx b / N)) the output spectrum is
 *     rows:     row p = 0 .. m - 1 takes source row src(p) = p for p < m div 2 and src(p) = M - m + p for every other p: the
 *               upper block is the LAST ceil(m / 2) source rows, so for odd m the middle row comes from the signed frequency
 *               -(m + 1) / 2.  This is the reference's slicing rule (src/image.py: F[0 : m // 2] and F[-m // 2 :]), kept exactly;
 *     columns:  kx = 0 .. n div 2 with weight w = 1 for kx = 0 and for the Nyquist column of an even n, 2 for every other one;
 * and the result is the real part of the inverse transform on the m x n grid times 1 / (M N) (the reference's (m n) / (M N)
 * folded into the 1 / (m n) of the inverse).  Equivalently, with
 *     Ry[i][a] = sum_p exp(2 pi i p i / m) exp(-2 pi i src(p) a / M),    Kx[b][j] = sum_kx w_kx exp(2 pi i kx (j / n - b / N)),
 *     out = (Re Ry  X  Re Kx  -  Im Ry  X  Im Kx) / (M N).
 *
 * tvae_image_resample does not build these tables: it is a GENERIC batched sandwich product
 *     out[b] = scale (Ar Xwin_b Br - Ai Xwin_b Bi),
 * the tables the caller's, row-major fp32, Ar and Ai [m][M], Br and Bi [N][n]; Ai = NULL together with Bi = NULL skips the
 * second term (one of them NULL alone is rejected).  tvae.tables.resample_tables builds the four tables of the downsample in
 * fp64 and rounds them once.  Arithmetic: fp32 FMA chains on the fp32 matrix pipe in a fixed order (first over the
 * window's rows, then over its columns in chunks of 64, the Ai / Bi product after the Ar / Br product of a chunk), the
 * scale applied once at the store.  No atomics: every output is a pure function of the inputs, bitwise reproducible, and
 * out[b] depends on image b and the tables only, not on B or the other images.  Nothing outside the window is read.
 * out must not overlap X or a table.
 *
 * Normalize.  Images X[B][n][m] (n rows, m columns).  The mask is (n / 2 - i)^2 + (m / 2 - j)^2 >= radius^2 for pixel (i, j):
 * the centre is (n / 2, m / 2), NOT ((n - 1) / 2, ..) (the reference's); evaluated exactly in fp64.  radius <= 0 means the
 * default, min(n, m) / 2.  mu = the mean over the masked pixels and sigma = their population (ddof = 0) standard deviation,
 * both in fp64, sigma in TWO passes (mu first, then sum (x - mu)^2: the sum-of-squares form fails on raw stacks whose mean
 * dwarfs their spread, the case this exists for).  Each pixel is (x - mu) / sigma formed in fp64 and rounded to fp32 once;
 * stats[b] = (mu, sigma) in fp64.  IEEE results stand: an empty mask gives NaN throughout, sigma = 0 gives +-inf or NaN.
 * Partial sums are fp64, combined in a fixed order (per 4096 pixels: per-thread sums in ascending pixel order and a fixed tree;
 * the groups of an image ascending): bitwise reproducible, image b's results depend on image b only.  out may be X.
 *
 * Supported: 1 <= B <= 2^24; 1 <= m <= M <= 1024, 1 <= n <= N <= 1024 and the window inside the frame (resample); 1 <= n, m
 * <= 1024 (normalize); fewer than 2^31 workgroups (B ceil(m / 64) ceil(n / 64 or 128); B ceil(n m / 4096)); a finite radius; ws
 * and stats 8-byte aligned.  Anything else returns hipErrorInvalidValue (1) and writes nothing, and the query returns 0. */

/* out[B][m][n] */
int tvae_image_resample(const float* X, const float* Ar, const float* Ai, const float* Br, const float* Bi, float* out,
                        int B, int H, int W, int r0, int c0, int M, int N, int m, int n, float scale,
                        tvae_stream_t stream);

/* floats of workspace of tvae_image_normalize: three fp64 partials per group of 4096 pixels.  0 for unsupported arguments. */
long tvae_image_normalize_ws_floats(int B, int n, int m);

/* X[B][n][m] -> out[B][n][m] (may be X), stats[B][2] (fp64) */
int tvae_image_normalize(const float* X, float* out, double* stats, float* ws, long ws_floats, int B, int n, int m,
                         float radius, tvae_stream_t stream);

/* ---- CTF: a real transfer function per image, the Fourier filter of a stack with it, and its per-class power ---------------
 *
 * Frequencies and shapes.  Square planes n x n, R = n / 2 + 1 (integer division).  ky = 0 .. n - 1 and kx = 0 .. R - 1 in the
 * order of numpy's fftfreq; ks(ky) is the signed frequency (ky for ky < (n + 1) / 2, ky - n for every other one);
 * q = (ks(ky)^2 + kx^2) / n^2, formed in fp64 from the exact integer numerator.
 *
 * Transfer function from five fp64 coefficients per plane, coef[B][5] = (c0, c1, c2, c3, c4):
 *     t = c2 q + c3 q^2   (turns, fp64),      H = (c0 sin 2 pi t + c1 cos 2 pi t) exp(-c4 q).
 * t is reduced to t - rint(t) in fp64 before anything is rounded to fp32; sin, cos and exp are each within 2 ulp of fp32 (as
 * built: sin and cos in fp64, c0 sin + c1 cos rounded to fp32 once, exp in fp32).  Contract:
 *     |H_gpu - H_fp64| <= 8 2^-24 (|c0| + |c1|)      (for c4 q >= 0).
 * mode = 1 replaces H by its sign: H < 0 gives -1, anything else +1.
 * For a contrast transfer function tvae.ctf.coefficients builds the row from the reference's eight-column table exactly as
 * src/ctf.py calls compute_2d_ctf: dfu = dfv = defocus 1e4, V = 1000 voltage, lambda = 12.2639 / sqrt(V + 0.97845e-6 V^2),
 * w = ampcont / 100, a = apix scale, c0 = sign sqrt(1 - w^2), c1 = -sign w, c2 = -0.5 df lambda / a^2,
 * c3 = 0.25 (cs 1e7) lambda^3 / a^4, c4 = bfactor / (4 a^2); sign = -1 is the model's convention (the filter the reference
 * trains with is -fftshift(Re ifft2(c))).  Astigmatism (dfdiff, dfang) is IGNORED, as the reference ignores it (it passes
 * dfu = dfv): H depends on q alone, which is also what lets the filter commute with the in-plane rotation of the alignment.
 *
 * Filter.  For a real plane x with X = DFT(x) on the half spectrum,
 *     out[i][j] = (1 / n^2) sum_ky sum_kx w_kx Re( H(ky, kx) X(ky, kx) exp(2 pi i (ky i + kx j) / n) ),
 * w_kx = 1 for kx = 0 and for the Nyquist column of an even n, 2 for every other one.  A direct DFT in four stages (rows,
 * columns, columns back, rows back) on the fp32 matrix pipe, the twiddles from a table of n entries whose argument
 * (i k) mod n is reduced in integers (each entry within an ulp), fp32 FMA chains in a fixed ascending order, H w applied to
 * the spectrum in one rounding, 1 / n^2 at the store.  No atomics: bitwise reproducible, and out[b] depends on plane b and its
 * H only, not on B.  One workgroup owns a plane from load to store.  n <= 128: the spectrum stays in LDS, and with coef
 * neither it nor H is ever in memory; n > 128: the spectrum goes through the plane's own part of the workspace, the same
 * launch whatever B is.
 *
 * Power.  tvae_ctf_power follows the order / seg rules of tvae_class_average (the section above states them): entries of
 * `order` outside [0, N) are skipped and not counted, seg is replaced on the device by min(max(0, seg[0], ..., seg[k]), N);
 * D[k] = the sum over the valid members of class k of H_i^2, H_i the fp32 value above (mode 0), squared and added in fp64 in
 * ascending position within the class.  No atomics; class k's result is independent of the other classes and of K.
 *
 * Supported: 2 <= n <= 1024, 1 <= B, N <= 2^24, 1 <= K <= 65535, fewer than 2^31 workgroups (N ceil(n R / 256) for
 * tvae_ctf_eval, K ceil(n R / 256) for tvae_ctf_power), mode 0 or 1, coef, D and ws 8-byte aligned.  Anything else returns
 * hipErrorInvalidValue (1) and writes nothing, and the query returns 0. */

/* H[N][n][R] fp32; mode 0 value, 1 sign */
int tvae_ctf_eval(const double* coef, float* H, int N, int n, int mode, tvae_stream_t stream);

/* floats of workspace of tvae_fourier_filter: n > 128: two complex buffers of n x (R | 1) per plane, 4 n (R | 1) B; n <= 128:
 * 2 (one 8-byte word that is never touched: 0 stays the answer for unsupported arguments). */
long tvae_fourier_filter_ws_floats(int B, int n);

/* X plane b at X + b * x_stride (x_stride = 0: one plane for all, else >= n n); exactly one of coef [B][5] and Hp (plane b at
 * Hp + b * h_stride, 0 = shared, else >= n R) is non-NULL; out[B][n][n] may be X itself (same base, x_stride = n n),
 * otherwise must not overlap it (an overlap is rejected). */
int tvae_fourier_filter(const float* X, long x_stride, const double* coef, const float* Hp, long h_stride, float* out,
                        float* ws, long ws_floats, int B, int n, int mode, tvae_stream_t stream);

/* D[K][n][R] fp64 = sum over the valid members of class k of H_i^2, counts[K] (int32) their number */
int tvae_ctf_power(const double* coef, const int* order, const int* seg, double* D, int* counts, int N, int K, int n,
                   tvae_stream_t stream);

/* ---- Radial spectra: the windowed ring power of a stack, its per-group sums, and a radial filter per group ---------------------
 *
 * Ring-indexed quantities of a stack's spectrum: the power is read per ring (a noise model for whitening), the filter is
 * written per ring (whitening, a low-pass at the FRC crossing, the FRC weight).  Planes, frequencies, ks(ky), the Hermitian
 * weights w_kx and the transform are those of the CTF section; the kernels run the SAME stage code as tvae_fourier_filter.
 *
 * Rings.  The ring of (ky, kx) is the integer rule of tvae_class_frc, (2r - 1)^2 <= 4 (ks^2 + kx^2) < (2r + 1)^2 for r >= 1
 * and r = 0 for 4 (ks^2 + kx^2) < 1, extended over the WHOLE plane, corners included: Rr = tvae_radial_rings(n) =
 * 1 + ring(h, h) with h = n / 2 (integer division) rings; 92 for n = 128 and 129, 46 for 64 and 65, 2 for n = 2 and 3.
 * Rings 0 .. n / 2 are the rings of tvae_class_frc.
 *
 * tvae_ring_power.  With m the soft mask of tvae_class_frc (centre ((n - 1) / 2, (n - 1) / 2), the same mask_radius /
 * mask_edge rules and rejections) the window is w = 1 - m for background = 1 (the noise outside the particle) and w = m for
 * background = 0; mask_radius <= 0 means w = 1 everywhere for both.  demean = 1: mu = sum w x / sum w in fp64 in a fixed
 * order (per-thread sums over the pixels tid, tid + 256, ... ascending, then the fixed tree of tvae_image_normalize);
 * (x - mu) is rounded to fp32 once and multiplied by w in fp32; an all-zero window gives the IEEE result, NaN.  demean = 0:
 * x w in fp32.  Transform: rows to the half spectrum, then columns (stages 1 and 2 of the filter).
 *     power[b][r] = sum over ring r of the FULL plane of |F(ky, kx)|^2 = sum over the half spectrum of w_kx |F|^2,
 * each |F|^2 formed in fp64 from the fp32 coefficient, added in fp64 in ascending ky index, then ascending kx (the order of
 * tvae_class_frc).  The raw sum: dividing by the coefficients of a ring and by sum w^2 is the caller's (neither depends on the
 * image; tvae.spectrum.ring_power does it).  No atomics: bitwise reproducible, power[b] depends on plane b only, not on B; a
 * NaN stays in its plane's row.  One workgroup owns a plane; n <= 128: the spectrum is never in memory; n > 128: it goes
 * through the plane's own part of the workspace.  Not bit for bit the sums[p][r][1] of tvae_class_frc (another kernel,
 * another order inside a coefficient).
 *
 * tvae_ring_power_groups follows the order / seg rules of tvae_ctf_power word for word: entries of `order` outside [0, N) are
 * skipped and not counted, seg is replaced on the device by min(max(0, seg[0], ..., seg[k]), N).  sums[k][r] = the fp64 sum
 * of power[i][r] over the valid members i of group k in ascending position, counts[k] their number.  A thread owns one
 * (k, r); no atomics; group k is independent of K and of the other groups; a non-finite row stays in its own group.
 *
 * tvae_radial_filter is tvae_fourier_filter with a third source of H: g = group ? group[b] : 0 and p = prof + g Rr,
 *     interp = 0 (nearest):  H(ky, kx) = p[ring(ky, kx)] by the integer rule;
 *     interp = 1 (linear):   s = sqrt((double)(ks^2 + kx^2)), r0 = min((int)floor(s), Rr - 2), t = s - r0,
 *                            H = (float)(p[r0] + (p[r0 + 1] - p[r0]) t), one fused multiply-add in fp64, rounded once
 *                            (Rr = 2: r0 = 0).
 * H is formed in registers; neither it nor the spectrum is in memory for n <= 128.  Everything else is the filter's: four
 * stages, H w applied in one rounding, 1 / n^2 at the store.  With interp = 0 the result is bit for bit that of
 * tvae_fourier_filter given Hp planes expanded from the same profile.  A g outside [0, G) makes that plane's output exact
 * zeros.  out may be X itself (same base, x_stride = n n); any other overlap of out and X is rejected.
 *
 * Supported: 2 <= n <= 1024, 1 <= B, N <= 2^24, 1 <= K, G <= 65535, 1 <= Rr <= tvae_radial_rings(1024) = 725
 * (tvae_ring_power_groups), x_stride 0 or >= n n, background, demean and interp 0 or 1, a finite mask with mask_edge >= 0,
 * power, sums and ws 8-byte aligned, ws_floats at least the query's.  Anything else returns hipErrorInvalidValue (1) and
 * writes nothing, and the queries return 0. */

/* rings of the whole plane, 1 + ring(n / 2, n / 2).  0 for unsupported n. */
int tvae_radial_rings(int n);
/* floats of workspace of tvae_ring_power: those of tvae_fourier_filter (n > 128: 4 n (R | 1) B; n <= 128: 2).  0 for
 * unsupported arguments. */
long tvae_ring_power_ws_floats(int B, int n);

/* X plane b at X + b * x_stride (0: one plane for all) -> power[B][Rr] fp64 */
int tvae_ring_power(const float* X, long x_stride, double* power, float* ws, long ws_floats, int B, int n, float mask_radius,
                    float mask_edge, int background, int demean, tvae_stream_t stream);

/* power[N][Rr] fp64 -> sums[K][Rr] fp64, counts[K] (int32) */
int tvae_ring_power_groups(const double* power, const int* order, const int* seg, double* sums, int* counts, int N, int K,
                           int Rr, tvae_stream_t stream);

/* floats of workspace of tvae_radial_filter: those of tvae_fourier_filter.  0 for unsupported arguments. */
long tvae_radial_filter_ws_floats(int B, int n);

/* prof[G][Rr] fp32, group[B] (int32) or NULL (group 0 for every plane); out[B][n][n] */
int tvae_radial_filter(const float* X, long x_stride, const float* prof, const int* group, float* out, float* ws,
                       long ws_floats, int B, int n, int G, int interp, tvae_stream_t stream);

/* ---- Eigenimages of the aligned classes: the class covariance applied to a block of vectors, no aligned copy --------------
 *
 * Shared definitions.  Y[N][C][n][n], theta[N], dx[N][2], t_scale, order[N] and seg[K + 1] exactly as for tvae_class_average
 * (the section above): the same sampling and zero border, the same out-of-frame rule (exact 0), `order` entries outside
 * [0, N) are skipped, and seg is replaced on the device by min(max(0, seg[0], ..., seg[k]), N).
 * mean[K][C][n][n] is the caller's class averages (of tvae_class_average, the avg of tvae_class_halves, or CTF-corrected ones).
 * V[K][J][C][n][n] is a block of J vectors per class, 1 <= J <= TVAE_EIGEN_MAX_COMPONENTS.
 * Mask: that of tvae_class_frc at the canonical pixel p = (i, j): the distance from ((n - 1) / 2, (n - 1) / 2) and the mask in
 * fp64, rounded to fp32 once; mask_radius <= 0 means no mask (m = 1), mask_edge = 0 a hard edge; a non-finite radius or edge
 * and a negative edge are rejected.  It is built once per call into the workspace.
 * Residual of position q of `order`, a valid member of class k, at (ch, p):
 *     a = the bilinear sample of image order[q] (A of the section above),   r = a - mean[k][ch][p]   (an fp32 subtraction),
 *     d_q(ch, p) = m(p) * r                                                                            (an fp32 product).
 * An image wholly out of frame has a = 0 exactly, so d = -m * mean rounded once: NaN, +-inf and huge poses included.
 *
 * tvae_class_project: coef[q][j] = sum_{ch,p} d_q(ch, p) V[k][j][ch][p] and norm2[q] = sum d_q^2, rows indexed by the POSITION
 * q in `order`, not by image.  Each is one fp32 FMA chain per thread followed by a fixed tree, the order of yy of
 * tvae_pose_refine: thread t of 256 takes the pixels t, t + 256, ... of channel 0, then of channel 1, ... in one chain
 * acc = fma(d, V, acc) (acc = fma(d, d, acc) for norm2) from 0; the 256 partial sums are then added as
 * s[t] += s[t + w] for w = 128, 64, ..., 1.  The longest chain of additions an output passes through is
 * C ceil(n n / 256) + 8.  A skipped entry and a position outside the cleaned [seg[0], seg[K]) get a row of exact zeros.  Row q
 * is a pure function of its image, its pose, mean[k], V[k] and the mask: not of N, K, the other rows or the launch (a workgroup
 * takes four consecutive positions and reuses V between those of one class; no chain changes with it).
 *
 * tvae_class_backproject: W[k][j][ch][p] = sum over the valid positions q of class k of coef[q][j] d_q(ch, p), and counts[k] the
 * number of valid members.  A class is cut into chunks of tvae_class_eigen_chunk members counted from the class's own first
 * position (a build constant, 128: four times the chunk of the averages, because a slot holds J planes).  Per chunk and
 * (j, ch, p) one fp32 chain acc = fma(coef[q][j], d_q, acc) in ascending position from 0, the sample d_q taken once for all
 * J; a second launch adds the chunks of a class in fp64 in ascending order and rounds to fp32 once.  Chunk c of class k owns
 * the slot floor(s_k / chunk) + k + c.  An empty class gives zeros.  Every output of class k depends only on class k's ordered
 * member list, those members' images, poses and coefficients and mean[k]: not on the other classes, not on K.
 * The workspace holds J C n n floats per slot, N / chunk + K slots: at N = 100 000, K = 10, C = 1, n = 128 and J = 8 that is
 * 791 slots of 512 KB, 415 MB (the chunk of the averages would take 1.6 GB).
 *
 * Both: no atomics, bitwise reproducible; no allocation, no synchronisation.  Supported: the range of tvae_class_average,
 * 1 <= J <= 16, K J C ceil(n n / 256) < 2^31, the mask rules above, ws 8-byte aligned and at least the queried size, and no
 * output (coef, norm2, W, counts, the used part of ws) overlapping an input or another output.  Anything else returns
 * hipErrorInvalidValue (1) and writes nothing, and the queries return 0. */

#define TVAE_EIGEN_MAX_COMPONENTS 16

/* floats of workspace of tvae_class_project: the cleaned seg (K + 1 int32 words, padded to a multiple of 4) and the mask
 * (n n).  0 for unsupported arguments. */
long tvae_class_project_ws_floats(int N, int K, int C, int n, int J);
/* floats of workspace of tvae_class_backproject: the cleaned seg and one member count per slot (int32 words, padded to a
 * multiple of 4), the mask (n n) and J C n n partial sums for each of N / chunk + K slots.  0 for unsupported arguments. */
long tvae_class_backproject_ws_floats(int N, int K, int C, int n, int J);
/* members per chunk of tvae_class_backproject (a constant of the build, 128).  0 for unsupported arguments. */
int tvae_class_eigen_chunk(int N, int K, int C, int n, int J);

/* coef[N][J], norm2[N] (may be NULL): rows by position in `order` */
int tvae_class_project(const float* Y, const float* theta, const float* dx, const int* order, const int* seg,
                       const float* mean, const float* V, float* coef, float* norm2, float* ws, long ws_floats, int N, int C,
                       int n, int K, int J, float t_scale, float mask_radius, float mask_edge, tvae_stream_t stream);

/* W[K][J][C][n][n], counts[K] (int32); coef[N][J] by position in `order`, as tvae_class_project writes it */
int tvae_class_backproject(const float* Y, const float* theta, const float* dx, const int* order, const int* seg,
                           const float* mean, const float* coef, float* W, int* counts, float* ws, long ws_floats, int N,
                           int C, int n, int K, int J, float t_scale, float mask_radius, float mask_edge,
                           tvae_stream_t stream);

/* ---- Maximum-likelihood class averages: the posterior over the candidates and the weighted aligned average -------------------
 *
 * The soft form of the averaging loop.  tvae_pose_classify gives every image one class and one pose, the arg-max; here every
 * image contributes to every (class, pose) it is compatible with, with its posterior weight under white Gaussian noise of
 * variance sigma2 per pixel.  The tables num, pp [N][M][NA][NS][NS], yy [N] and cand [N][M] are those of tvae_pose_classify
 * (NA = 2A + 1, NS = 2S + 1), theta, dx, n, t_scale and dtheta its poses and grid; logprior[K] (fp64) the log prior of every
 * class, NULL meaning 0 for all of them.
 *
 * tvae_pose_posterior.  Candidates: j = ((m NA + a') NS + sy') NS + sx' with a' = a + A, sy' = sy + S, sx' = sx + S, J = M NA NS^2
 * of them per image.  In fp64, every operation rounded on its own,
 *     r_j = ((double)yy - 2 (double)num_j) + (double)pp_j        (the squared residual |Y - P_j|^2),
 *     h = 0.5 / (double)sigma2,      l_j = logprior[cand[i][m]] - r_j h.
 * A candidate is LIVE if cand[i][m] is inside [0, K) and l_j is finite: a -inf prior, a NaN table entry and an invalid slot take
 * it out.  With L the maximum of the live l_j and e_j = exp(l_j - L) (0 for a candidate that is not live):
 *     E_m = sum of e_j over slot m,   R_m = sum of e_j r_j over slot m,   Z = sum_m E_m,   w_j = e_j / Z,
 *     lse[i] = L + log Z,    r2[i] = (sum_m R_m) / Z  (= sum_j w_j r_j),    resp[i][m] = (float)(E_m / Z).
 * Order of addition, a function of (M, A, S) only: within slot m thread t of 256 adds the candidates c = t, t + 256, ... of the
 * slot (c = j - m NA NS^2) in one chain from 0, the 256 sums are then added by a binary tree (t and t + 128, then t and t + 64,
 * ...), the order of yy of tvae_pose_refine; Z and sum R_m add the slots in ascending m.  Everything is fp64; resp is rounded
 * to fp32 once.
 * Selection: the live candidates ranked by l descending, then j ascending; the first P' = min(P, live) are kept, W = the sum of
 * their w_j in rank order.  For the kept rank p: ent_idx[i][p] = j, ent_cls[i][p] = cand[i][m], ent_w[i][p] = (float)(w_j / W),
 * and ent_theta[i][p], ent_dx[i][p] the pose of the candidate (a, sy, sx) by the pose update of tvae_pose_refine, bit for bit
 * what tvae_pose_classify writes for that candidate (an index that is 0 copies its part of the pose bit for bit);
 * kept[i] = (float)W.  For the ranks p >= P': ent_idx = ent_cls = -1, ent_w = 0 and the pose is the image's own, bit for bit.
 * An image with no live candidate gets lse = r2 = kept = 0, zeros in resp and empty entries only.
 * One workgroup per image; l_j stays in LDS for J <= 4096 and is formed again by the same operations otherwise: the same bits.
 * No atomics; every output is bitwise reproducible, and the outputs of image i depend on its own rows only.
 *
 * Supported: 1 <= N <= 2^24, 2 <= n <= 128, 1 <= K <= 65535, 1 <= M <= 64, 0 <= A <= 32, 0 <= S <= 8 (the range of
 * tvae_pose_classify), 1 <= P <= TVAE_POSTERIOR_MAX_KEEP, t_scale and sigma2 finite and > 0, dtheta finite, logprior (where
 * given), lse and r2 8-byte aligned, and no output overlapping an input or another output.  Anything else returns
 * hipErrorInvalidValue (1) and writes nothing.
 *
 * tvae_class_average_weighted.  E entries, already grouped by class: class k is the entries [seg[k], seg[k + 1]), seg[K + 1]
 * cleaned on the device as for tvae_class_average with E as the upper bound, min(max(0, seg[0], ..., seg[k]), E).  Entry e
 * resamples image img[e] of Y[N][C][n][n] at the pose (theta_e[e], dx_e[e][2]) with the sampling, the zero border and the
 * out-of-frame rule of tvae_class_average (a_e, exact zeros out of frame), and carries the weight w[e].  An entry is LIVE if
 * img[e] is inside [0, N) and w[e] is finite and > 0; an entry that is not contributes to nothing and nothing of Y is read for
 * it.  A live entry whose pose is out of frame (NaN, +-inf and huge poses among them) contributes exact zeros to the sum and
 * its weight to the denominator, as an out-of-frame member counts in tvae_class_average.
 * A class is cut into chunks of tvae_class_average_weighted_chunk entries (a build constant, 128: E is several times N and a
 * slot is one C n n plane) counted from the class's own first entry; chunk c of class k owns the slot
 * floor(s_k / chunk) + k + c.  Per chunk and (ch, pixel) one fp32 chain acc = fma(w_e, a_e, acc) in ascending e from 0; per
 * chunk the fp64 sum of the live weights in ascending e, and the live count.  A second launch adds a class's chunks in ascending
 * order in fp64, S over the chains and W_k over the weights, and writes
 *     avg[k] = (float)(S / W_k) (zeros where W_k = 0),    wsum[k] = W_k (fp64),    counts[k] = the live entries.
 * No atomics; every output is bitwise reproducible, and the outputs of class k depend on class k's own entry list and the
 * images it names only: not on K, not on the other classes.
 *
 * Supported: 1 <= E <= 2^30, N, C, n and K as for tvae_class_average (1 <= N <= 2^24, 1 <= C <= 1024, 2 <= n <= 1024,
 * 1 <= K <= 65535, N C ceil(n n / 256) < 2^31), (E / chunk + K) C ceil(n n / 256) < 2^31, ws at least the queried size, ws and
 * wsum 8-byte aligned, no output (the used part of ws is one) overlapping an input or another output.  Anything else returns
 * hipErrorInvalidValue (1) and writes nothing, and the queries return 0. */

#define TVAE_POSTERIOR_MAX_KEEP 64

/* ent_idx, ent_cls [N][P] (int32), ent_theta [N][P], ent_dx [N][P][2], ent_w [N][P], resp [N][M], lse [N] and r2 [N] (fp64),
 * kept [N] */
int tvae_pose_posterior(const float* num, const float* pp, const float* yy, const int* cand, const double* logprior,
                        const float* theta, const float* dx, int* ent_idx, int* ent_cls, float* ent_theta, float* ent_dx,
                        float* ent_w, float* resp, double* lse, double* r2, float* kept, int N, int n, int K, int M, int A,
                        int S, int P, float t_scale, float dtheta, float sigma2, tvae_stream_t stream);

/* floats of workspace of tvae_class_average_weighted: the cleaned seg and one live count per chunk slot (int32 words, padded to
 * a multiple of 4), one fp64 weight sum per slot and the partial sums of E / chunk + K slots.  0 for unsupported arguments. */
long tvae_class_average_weighted_ws_floats(int E, int K, int C, int n);
/* entries per chunk (a constant of the build, 128).  0 for unsupported arguments. */
int tvae_class_average_weighted_chunk(int E, int K, int C, int n);

/* avg[K][C][n][n], wsum[K] (fp64), counts[K] (int32); ws holds tvae_class_average_weighted_ws_floats(E, K, C, n) floats */
int tvae_class_average_weighted(const float* Y, const int* img, const float* theta_e, const float* dx_e, const float* w,
                                const int* seg, float* avg, double* wsum, int* counts, float* ws, long ws_floats, int N, int E,
                                int C, int n, int K, float t_scale, tvae_stream_t stream);

/* ---- CTF in the template: the norm of the CTF-filtered template and the weighted per-class power of the CTF ------------------
 *
 * The pose searches above score an image against the rendered class average as if no transfer function lay between them.
 * Under the model Y_i = H_i (*) P_j + noise, H_i the real, radially symmetric transfer function of tvae_ctf_eval (mode 0) of
 * image i and (*) the circular convolution of the CTF section's filter, the squared residual is
 *     |Y_i - H_i (*) P_j|^2 = |Y_i|^2 - 2 <H_i (*) Y_i, P_j> + |H_i (*) P_j|^2.
 * H_i is real and even, so the filter is self-adjoint: the middle term is the num table of tvae_pose_classify run on the
 * stack that tvae_fourier_filter (coef, mode 0) has already filtered.  The last term is what tvae_template_ctf_power forms;
 * the M-step of the soft average under this model is a Wiener form whose denominator tvae_ctf_power_entries forms.
 * The shift of a candidate enters num through windows of the extended template but enters the last term circularly (a
 * circular shift is a phase factor, which |.|^2 drops): the two agree exactly while the masked support of the template moved
 * by the shift stays inside the frame, and differ by what leaves the frame otherwise.
 *
 * tvae_template_ctf_power.  theta[N], dx[N][2], cand[N][M], ref[K][C][n][n], A, t_scale, dtheta, mask_radius and mask_edge as
 * for tvae_pose_classify; coef[N][5] as for tvae_ctf_eval.  For image i, slot m with k = cand[i][m] and angle index
 * a' = 0 .. 2A (NA = 2A + 1), T is the template of tvae_pose_refine of reference k at the angle theta[i] + (a' - A) dtheta on
 * the frame r, q = 0 .. n - 1, its mask included: the same device functions build it, so its pixels are bit for bit the centre
 * window of that kernel's extended template.  Per channel F = DFT(T) by stages 1 and 2 of the filter (rows to the half
 * spectrum, then columns: the code of tvae_ring_power, fp32 chains on the matrix pipe), H = H_i(ky, kx) the fp32 value of
 * tvae_ctf_eval, mode 0, formed in registers, and
 *     ppc[i][m][a'] = (float)( (1 / n^2) sum_ch sum_ky sum_kx w_kx (double)H^2 (double)|F|^2 ).
 * Order: (double)H (double)H is exact, |F|^2 = re re + im im is formed in fp64 from the fp32 coefficient (the squares are
 * exact, the sum is one rounding), their product is one rounding and w_kx is exact.  Thread t of 256 adds the coefficients
 * e = ky R + kx = t, t + 256, ... (ascending ky index, then kx) of channel 0, then of channel 1, ... in ONE fp64 chain from 0; the
 * 256 chains are added by the fixed tree of tvae_ring_power's demean (s[t] += s[t + w] for w = 128, 64, ..., 1); the total is
 * divided by (double)(n n) and rounded to fp32 once.
 * One workgroup owns one (image, slot, angle) from template to sum; the template plane and the half spectrum stay in LDS (the
 * budget of tvae_ring_power: 134 144 bytes at n = 128), and neither H, T nor the spectrum is ever in memory.  The workspace is
 * the 2-float word of tvae_fourier_filter and is never touched.  No atomics: bitwise reproducible; row i depends on image i's
 * pose, its row of candidates, coef[i] and the references that row names only: not on N, K or the launch.
 * A slot outside [0, K) gives zeros and nothing of ref is read for it.  A pose that puts every sample out of frame (NaN, +-inf
 * and huge poses among them) gives exact 0 (for a finite H).  A non-finite coef row gives that image's IEEE results and touches
 * no other row.
 *
 * Supported: 1 <= N <= 2^24, 1 <= C <= 16, 2 <= n <= 128, 1 <= K <= 65535, 1 <= M <= 64, 0 <= A <= 32 (the range of
 * tvae_pose_classify without S), N M NA < 2^31, t_scale finite and > 0, dtheta finite, the mask rules of tvae_class_frc, coef
 * and ws 8-byte aligned, ws_floats at least the query's, no output overlapping an input.  Anything else returns
 * hipErrorInvalidValue (1) and writes nothing, and the query returns 0.
 *
 * tvae_ctf_power_entries.  E entries grouped by class with img[e], w[e] and seg[K + 1] exactly as for
 * tvae_class_average_weighted: seg is cleaned on the device with E as the bound, min(max(0, seg[0], ..., seg[k]), E), and an
 * entry is LIVE if img[e] is inside [0, N) and w[e] is finite and > 0.
 *     D[k][ky][kx] = sum over the live entries of class k in ascending e of (double)w_e (double)H^2,
 * H the fp32 value of tvae_ctf_eval (mode 0) of image img[e], (double)H (double)H exact, its product with the weight one
 * rounding, the sum fp64; wsum[k] = the fp64 sum of the live weights in ascending e and counts[k] their number.  A thread owns
 * one (k, coefficient).  No atomics; class k is independent of K and of the other classes.  With unit weights over a partition
 * D is bit for bit that of tvae_ctf_power.
 *
 * Supported: the range of tvae_ctf_power (2 <= n <= 1024, 1 <= N <= 2^24, 1 <= K <= 65535, K ceil(n R / 256) < 2^31) with
 * 1 <= E <= 2^30, coef, D and wsum 8-byte aligned, no output overlapping an input or another output.  Anything else returns
 * hipErrorInvalidValue (1) and writes nothing. */

/* floats of workspace of tvae_template_ctf_power: 2 (one 8-byte word that is never touched).  0 for unsupported arguments. */
long tvae_template_ctf_power_ws_floats(int N, int C, int n, int M, int A);

/* ppc[N][M][NA] */
int tvae_template_ctf_power(const float* theta, const float* dx, const int* cand, const float* ref, const double* coef,
                            float* ppc, float* ws, long ws_floats, int N, int C, int n, int K, int M, int A, float t_scale,
                            float dtheta, float mask_radius, float mask_edge, tvae_stream_t stream);

/* D[K][n][R] (fp64), wsum[K] (fp64), counts[K] (int32) */
int tvae_ctf_power_entries(const double* coef, const int* img, const float* w, const int* seg, double* D, double* wsum,
                           int* counts, int N, int E, int K, int n, tvae_stream_t stream);

/* ---- Selection of a hard pose search from its tables: the template power per candidate or per angle ---------------------------
 *
 * tvae_pose_classify forms the tables num, pp, yy and selects from them in one call.  Under the model of the section above the
 * three terms come from three places -- num from tvae_pose_classify (or tvae_pose_refine, the M = 1 layout) on the stack
 * filtered with H_i, the template power from tvae_template_ctf_power, which does not depend on the shift, and yy from the raw
 * stack -- so the selection is an entry point of its own that takes the template power per angle as it is written, without a
 * copy expanded over the NS^2 shifts.  theta[N], dx[N][2], cand[N][M] (int32), n, K, M, A, S, t_scale and dtheta as for
 * tvae_pose_classify; num[N][M][NA][NS][NS]; yy[N]; pp[N][M][NA] when pp_per_shift = 0 and [N][M][NA][NS][NS] when it is 1.
 *
 * Per candidate.  The candidate with the flat index e = (a' NS + sy') NS + sx' of slot m (a' = 0 .. 2A, sy', sx' = 0 .. 2S; the
 * centre is a' = A, sy' = sx' = S) has the score of tvae_pose_refine from num[i][m][e], p and yy[i]: num / sqrt(p yy) in fp64
 * from the three fp32 words (product, square root and quotient each correctly rounded), rounded to fp32 once; exactly 0 where
 * p or yy is 0.  p = pp[i][m][a'] when pp_per_shift = 0 and pp[i][m][e] when it is 1.
 *
 * Per slot.  The rule of tvae_pose_refine, stated without an order of visits: among the candidates whose score is finite the
 * largest score wins; among equal largest scores the centre wins if it is one of them, and otherwise the lowest flat index
 * (+0 and -0 are equal).  score[i][m] = (sc, sb): sb the winner's score, sc the centre's, -inf if the centre's is not finite.
 * If no candidate is finite the slot reports (0, 0) and the centre.  Any parallel reduction under this order gives the same
 * bits as the serial visit of tvae_pose_refine.
 *
 * Across slots and outputs.  Those of tvae_pose_classify: the valid slots in ascending m, a later one wins only with a strictly
 * greater sb; cls_out[i] = cand[i][m*], best[i] = (m*, a, sy, sx) = (m*, a' - A, sy' - S, sx' - S), theta_out and dx_out by the
 * pose update of tvae_pose_refine (an index that is 0 copies its part of the pose bit for bit).  A slot outside [0, K) is
 * skipped: its scores are (0, 0) and nothing of its rows of num and pp is read.  An image with no valid slot keeps its pose bit
 * for bit and gets cls_out = cand[i][0], best = 0 and zero scores.  With pp_per_shift = 1 on the tables of one
 * tvae_pose_classify call every output is that call's bit for bit.
 *
 * One wavefront owns an image, four images a workgroup of 256; the lanes stride over the candidates of a slot, so the loads of
 * num are contiguous, and reduce with cross-lane shuffles.  No LDS, no atomics, no workspace: bitwise reproducible, and every
 * output of image i depends on row i of the inputs only: not on N or the launch.
 *
 * Supported: 1 <= N <= 2^24, 2 <= n <= 128, 1 <= K <= 65535, 1 <= M <= 64, 0 <= A <= 32, 0 <= S <= 8 (the range of
 * tvae_pose_classify without its channels), pp_per_shift 0 or 1, N M NA NS^2 < 2^40, t_scale finite and > 0, dtheta finite, no
 * output overlapping an input or another output.  Anything else returns hipErrorInvalidValue (1) and writes nothing. */

/* cls_out[N] (int32), best[N][4] = (m*, a, sy, sx) (int32), theta_out[N], dx_out[N][2], score[N][M][2] = (centre, best) */
int tvae_pose_select(const float* theta, const float* dx, const int* cand, const float* num, const float* pp, const float* yy,
                     int* cls_out, int* best, float* theta_out, float* dx_out, float* score, int N, int n, int K, int M, int A,
                     int S, int pp_per_shift, float t_scale, float dtheta, tvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TVAE_CLUSTER_H */
