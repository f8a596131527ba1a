"""Clustering of the content latents and the metrics TARGET-VAE is judged by (reference clustering_*.py).

k-means is the hot path: the reference's KMeans(n_init=100) is 100 restarts of up to 300 Lloyd iterations.  Here all
restarts advance together on the HIP kernels of libtvae_cluster.so (tvae._cluster_lib; include/tvae_cluster.h): one
assign launch labels every point of every restart and leaves ordered per-cluster partial sums, one update launch turns
them into the new centroids, the inertia and the centre shift.  No float atomics: a run is bitwise reproducible and a
restart's trajectory does not depend on which other restarts share the launch.  There is no CPU fallback.

Ward agglomerative clustering (the default of the particles and galaxy scripts) runs on the same library: ward_linkage
merges all reciprocal nearest neighbours per round from sizes and centroids alone, ward_cut numbers the flat clusters
as sklearn does.  The reference's sklearn path stays for host arrays (agglomerative).

The metrics (cluster_acc, circcorrcoef, measure_correlations) are host code like the reference's.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _cluster_lib as CL
from ._lib import TvaeHipError

KMeansResult = namedtuple('KMeansResult', 'labels centers inertia n_iter all_inertia best')
WardResult = namedtuple('WardResult', 'Z n_rounds')
MAX_RESTARTS = 65535                 # TVAE_KMEANS_MAX_RESTARTS of include/tvae_cluster.h
WARD_MAX_POINTS = 1 << 24            # cluster sizes are fp32 on the device, exact up to here
CHECK_EVERY = 8                      # iterations between two host reads of the per-restart `done` flags


def _feature_major(X):
    """X [N][d] -> (Xt [d][ldx], ldx): points along the contiguous index (the kernels' layout), ldx a multiple of 4."""
    N, d = X.shape
    ldx = (N + 3) // 4 * 4
    Xt = torch.zeros(d, ldx, dtype=torch.float32, device=X.device)
    Xt[:, :N] = X.t()
    return Xt, ldx


def _check_points(X, k):
    if not (CL.is_f32(X, contiguous=False) and X.dim() == 2):
        raise TvaeHipError('kmeans: X must be a CUDA fp32 [N][d] tensor (no CPU fallback)')
    N, d = X.shape
    if not (1 <= d <= 256 and 1 <= k <= 1024 and k <= N):
        raise TvaeHipError(f'kmeans: N={N}, d={d}, k={k} outside the supported range (d <= 256, k <= 1024, k <= N)')
    return N, d


def _check_restarts(R, N):
    if not (1 <= R <= MAX_RESTARTS and R * N < 2 ** 31):
        raise TvaeHipError(f'kmeans: n_init = {R} must be in [1, {MAX_RESTARTS}] and n_init * N = {R * N} below 2^31')


def kmeans_plusplus(X, n_clusters, n_init, seed=None, Xt=None):
    """Plain k-means++ seeding of n_init restarts at once -> C [n_init][k][d], every centre bitwise a row of X.

    The first centre is uniform, each further one is drawn with probability proportional to D^2, the squared distance
    to the nearest centre chosen so far (tvae_kmeans_mindist for all restarts in one launch, torch.multinomial under a
    torch.Generator seeded by `seed`).  This is the original algorithm, NOT sklearn's greedy variant, which tries
    2 + log(k) candidates per centre and keeps the best.  torch.multinomial limits N to 2^24 points."""
    N, d = _check_points(X, n_clusters)
    R, k = int(n_init), int(n_clusters)
    _check_restarts(R, N)
    if Xt is None:
        Xt, ldx = _feature_major(X)
    else:
        ldx = Xt.shape[1]
    g = torch.Generator(device=X.device)
    if seed is None:
        g.seed()
    else:
        g.manual_seed(int(seed))
    C = torch.empty(R, k, d, dtype=torch.float32, device=X.device)
    D = torch.full((R, N), float('inf'), dtype=torch.float32, device=X.device)
    idx = torch.randint(N, (R,), generator=g, device=X.device)
    for c in range(k):
        cnew = X[idx].contiguous()
        C[:, c] = cnew
        if c + 1 == k:
            break
        CL.call('tvae_kmeans_mindist', Xt, ldx, cnew, D, N, d, R)
        w = D + (D.sum(1, keepdim=True) == 0)             # every point already a centre: uniform
        idx = torch.multinomial(w, 1, generator=g).squeeze(1)
    return C


def kmeans(X, n_clusters, n_init=100, max_iter=300, tol=1e-4, seed=None, init=None):
    """Lloyd k-means with n_init restarts advancing together on the GPU.

    X: CUDA fp32 [N][d] (transposed once into the kernels' feature-major layout).  init: optional [n_init][k][d] tensor
    of explicit starting centroids (n_init is then its first dimension); otherwise k-means++ (kmeans_plusplus: plain D^2
    sampling, not sklearn's greedy-trials variant) under `seed`.

    A restart stops under sklearn's rules -- no label changed in an iteration, or centre shift sum ||dC||^2 <= tol *
    mean per-feature variance of X -- or at max_iter.  Its flag is raised on the device in the iteration that meets the
    rule and the kernels skip it from then on, so it is frozen bit for bit; the host reads the small flag array once
    every CHECK_EVERY iterations (one D2H copy) to learn whether every restart has finished.  One last assign pass over
    all restarts gives labels and inertia against the FINAL centroids (as KMeans.predict does in the reference scripts);
    the winner is the restart of lowest inertia.

    Returns KMeansResult(labels int64 [N], centers [k][d], inertia, n_iter, all_inertia [n_init], best)."""
    k = int(n_clusters)
    N, d = _check_points(X, k)
    X = X.contiguous()
    dev = X.device
    Xt, ldx = _feature_major(X)
    if init is not None:
        if not (torch.is_tensor(init) and init.dim() == 3 and tuple(init.shape[1:]) == (k, d)):
            raise TvaeHipError(f'kmeans: init must be [n_init][{k}][{d}]')
        C = init.to(device=dev, dtype=torch.float32).contiguous().clone()
    else:
        C = kmeans_plusplus(X, k, n_init, seed, Xt=Xt)
    R = C.shape[0]
    _check_restarts(R, N)
    ws_floats = CL.query('tvae_kmeans_ws_floats', N, d, k, R)
    if ws_floats <= 0:
        raise TvaeHipError(f'kmeans: N={N}, d={d}, k={k}, n_init={R} is not supported by libtvae_cluster.so')
    ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
    labels = torch.full((R, N), -1, dtype=torch.int32, device=dev)
    mind2 = torch.empty(R, N, dtype=torch.float32, device=dev)
    changed = torch.zeros(R, dtype=torch.int32, device=dev)
    inertia = torch.zeros(R, dtype=torch.float32, device=dev)
    shift = torch.zeros(R, dtype=torch.float32, device=dev)
    done = torch.zeros(R, dtype=torch.int32, device=dev)
    n_iter = torch.zeros(R, dtype=torch.int32, device=dev)
    tol_abs = (X.double().var(dim=0, unbiased=False).mean() * tol).float()        # stays on the device

    for it in range(int(max_iter)):
        n_iter += 1 - done
        CL.call('tvae_kmeans_assign', Xt, ldx, C, done, labels, mind2, changed, ws, ws_floats, N, d, k, R)
        CL.call('tvae_kmeans_update', ws, ws_floats, done, C, inertia, shift, N, d, k, R)
        done |= ((changed == 0) | (shift <= tol_abs)).to(torch.int32)             # frozen restarts keep their stale flags
        if (it + 1) % CHECK_EVERY == 0 and bool(done.all()):
            break
    # labels / inertia of every restart against its final centroids (the update runs on a scratch copy)
    done.zero_()
    CL.call('tvae_kmeans_assign', Xt, ldx, C, done, labels, mind2, changed, ws, ws_floats, N, d, k, R)
    CL.call('tvae_kmeans_update', ws, ws_floats, done, C.clone(), inertia, shift, N, d, k, R)
    best = int(torch.argmin(inertia))
    all_inertia = inertia.clone()
    return KMeansResult(labels[best].to(torch.int64), C[best].clone(), float(all_inertia[best]), int(n_iter[best]),
                        all_inertia, best)


def _check_ward_points(X):
    if not (CL.is_f32(X, contiguous=False) and X.dim() == 2):
        raise TvaeHipError('ward_linkage: X must be a CUDA fp32 [N][d] tensor (no CPU fallback)')
    N, d = X.shape
    if not (2 <= N <= WARD_MAX_POINTS and 1 <= d <= 256):
        raise TvaeHipError(f'ward_linkage: N={N}, d={d} outside the supported range (2 <= N <= 2^24, 1 <= d <= 256)')
    return N, d


def _check_finite(X):
    if not bool(torch.isfinite(X).all()):
        raise TvaeHipError('ward_linkage: X holds NaN or Inf')


def ward_linkage(X):
    """Ward linkage of the rows of X (CUDA fp32 [N][d]) on the GPU, without the N x N distance matrix.

    The Ward distance of two clusters depends on their sizes and centroids alone, w(A,B) = |A||B| / (|A|+|B|) *
    ||c_A - c_B||^2 (scipy's height is sqrt(2 w)), and Ward is a reducible linkage: two clusters that are each other's
    nearest neighbour belong to the final dendrogram.  A round is therefore tvae_ward_nn (all-pairs nearest neighbour
    of the M live centroids, O(M^2 d) work, O(M d) memory) and tvae_ward_merge (every reciprocal pair merged, the
    survivors compacted into the other half of a ping-pong buffer), then one D2H copy of the new M.  The kernels make w
    bitwise symmetric and send ties to the lowest index, so the lexicographically least pair at the global minimum is
    always reciprocal: every round merges something, and a round that does not raises instead of looping.

    X is centred first (per-feature mean in fp64 on the device; Ward is translation invariant) and must be finite: a
    NaN would break the progress guarantee, so it is refused before any launch.  The centroids are kept in fp64 beside
    the fp32 copy that the search reads, and the recorded heights are fp64: merges whose heights differ by less than an
    fp32 ulp (a few per thousand points) would otherwise sort, and so be numbered, differently from an fp64 linkage.

    Returns WardResult(Z, n_rounds): Z is the fp64 numpy [N-1][4] array of scipy.cluster.hierarchy.linkage (children
    min / max, height, size; rows sorted by height, ties in creation order; node N + r made by row r)."""
    N, d = _check_ward_points(X)
    _check_finite(X)
    dev = X.device
    X64 = X.double()
    ldc = (N + 3) // 4 * 4
    C64 = torch.zeros(2, d, ldc, dtype=torch.float64, device=dev)
    C64[0, :, :N] = (X64 - X64.mean(dim=0, keepdim=True)).t()
    Ct = torch.zeros(2, d, ldc, dtype=torch.float32, device=dev)
    Ct[0] = C64[0]
    cnt = torch.ones(2, ldc, dtype=torch.float32, device=dev)
    ids = torch.zeros(2, N, dtype=torch.int32, device=dev)
    ids[0] = torch.arange(N, dtype=torch.int32, device=dev)
    hmax = torch.zeros(2, N, dtype=torch.float64, device=dev)
    nn = torch.zeros(N, dtype=torch.int32, device=dev)
    nd = torch.zeros(N, dtype=torch.float32, device=dev)
    rec_ids = torch.zeros(N - 1, 2, dtype=torch.int32, device=dev)
    rec_hs = torch.zeros(N - 1, 2, dtype=torch.float64, device=dev)
    m_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    wsm_ints = CL.query('tvae_ward_merge_ws_ints', N, d)
    wsm = torch.empty(wsm_ints, dtype=torch.int32, device=dev)
    ws = None

    M, base, cur, rounds = N, 0, 0, 0
    while M > 1:
        need = CL.query('tvae_ward_nn_ws_floats', M, d)               # not monotone in M: the column split changes
        if need <= 0:
            raise TvaeHipError(f'ward_linkage: M={M}, d={d} is not supported by libtvae_cluster.so')
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.float32, device=dev)
        nxt = 1 - cur
        CL.call('tvae_ward_nn', Ct[cur], ldc, cnt[cur], nn, nd, ws, ws.numel(), M, d)
        CL.call('tvae_ward_merge', C64[cur], ldc, cnt[cur], ids[cur], hmax[cur], nn, C64[nxt], Ct[nxt], ldc, cnt[nxt],
                ids[nxt], hmax[nxt], rec_ids, rec_hs, m_dev, wsm, wsm_ints, M, d, N, base, N - 1)
        m_new = int(m_dev.item())
        if not 1 <= m_new < M:
            raise TvaeHipError(f'ward_linkage: round {rounds} merged nothing (M = {M} -> {m_new}); non-finite distances?')
        base += M - m_new
        M, cur, rounds = m_new, nxt, rounds + 1
    assert base == N - 1

    # creation order -> scipy's order: stable sort by height, temporary ids N + creation index -> N + rank
    order = torch.sort(rec_hs[:, 0], stable=True).indices
    rank = torch.empty_like(order)
    rank[order] = torch.arange(N - 1, device=dev)
    ch = rec_ids.to(torch.int64)
    ch = torch.where(ch >= N, N + rank[(ch - N).clamp_(min=0)], ch)[order]
    Z = torch.empty(N - 1, 4, dtype=torch.float64, device=dev)
    Z[:, 0] = ch.min(dim=1).values
    Z[:, 1] = ch.max(dim=1).values
    Z[:, 2:] = rec_hs[order]
    return WardResult(Z.cpu().numpy(), rounds)


def ward_cut(Z, n_clusters):
    """Flat clusters of a linkage matrix Z (scipy convention), numbered as sklearn's AgglomerativeClustering numbers
    them -> int64 labels [N].

    A min-heap of negated node ids starts with the root; n_clusters - 1 times its top node (the highest id = the
    last merge still whole) is split: the first child is pushed, the second one pushed while the top is popped.  Label
    i goes to the leaves under the i-th entry of the heap in its ARRAY order.  The labels reach the leaves by pointer
    jumping over the parent array (log2(depth) array operations, no Python loop over N)."""
    import heapq
    Z = np.asarray(Z)
    N = Z.shape[0] + 1
    k = int(n_clusters)
    if not (Z.ndim == 2 and Z.shape[1] == 4 and N >= 2):
        raise ValueError('ward_cut: Z must be an [N-1][4] linkage matrix')
    if not 1 <= k <= N:
        raise ValueError(f'ward_cut: n_clusters = {k} must be in [1, {N}]')
    children = Z[:, :2].astype(np.int64)
    heap = [-(2 * N - 2)]
    for _ in range(k - 1):
        a, b = children[-heap[0] - N]
        heapq.heappush(heap, -int(a))
        heapq.heappushpop(heap, -int(b))
    cut = -np.asarray(heap, dtype=np.int64)
    anc = np.arange(2 * N - 1, dtype=np.int64)                        # the root and the cut nodes point at themselves
    parent = np.arange(N, 2 * N - 1, dtype=np.int64)
    anc[children[:, 0]] = parent
    anc[children[:, 1]] = parent
    anc[cut] = cut
    while True:
        nxt = anc[anc]
        if np.array_equal(nxt, anc):
            break
        anc = nxt
    label_of = np.full(2 * N - 1, -1, dtype=np.int64)
    label_of[cut] = np.arange(k)
    labels = label_of[anc[:N]]
    assert (labels >= 0).all()
    return labels


def agglomerative(z_values, n_clusters):
    """Ward agglomerative clustering, the reference's default for particles and galaxy.  A CUDA tensor is clustered on
    the GPU (ward_linkage + ward_cut, the numbering of sklearn's fit_predict); a numpy array or a CPU tensor takes the
    reference's own host path, sklearn's AgglomerativeClustering, which builds the N (N - 1) / 2 distance matrix."""
    if torch.is_tensor(z_values) and z_values.is_cuda:
        return ward_cut(ward_linkage(z_values.float().contiguous()).Z, n_clusters)
    try:
        from sklearn.cluster import AgglomerativeClustering
    except ImportError as e:
        raise SystemExit('--clustering agglomerative on the host needs scikit-learn (not installed here); pass the '
                         'latents as a CUDA tensor, or use --clustering k-means') from e
    ac = AgglomerativeClustering(n_clusters=n_clusters, linkage='ward', compute_full_tree=True)
    return ac.fit_predict(_np(z_values))


def cluster_acc(y_true, y_pred):
    """Clustering accuracy under the best one-to-one relabelling (reference clustering_mnist.py:170-190).
    Returns (mapping, accuracy): mapping = linear_sum_assignment of the (true, predicted) contingency table."""
    from scipy.optimize import linear_sum_assignment
    y_true = np.asarray(y_true).astype(np.int64)
    y_pred = np.asarray(y_pred).astype(np.int64)
    assert y_pred.size == y_true.size
    D = max(y_pred.max(), y_true.max()) + 1
    w = np.zeros((D, D), dtype=np.int64)
    np.add.at(w, (y_true, y_pred), 1)
    mapping = linear_sum_assignment(w.max() - w)
    return mapping, w[mapping[0], mapping[1]].sum() / y_pred.shape[0]


def circcorrcoef(a, b):
    """Circular correlation coefficient of Jammalamadaka & SenGupta (what the reference takes from astropy.stats), in
    fp64 over all elements: mu = atan2(sum sin, sum cos), rho = sum sin(a - mu_a) sin(b - mu_b) /
    sqrt(sum sin^2(a - mu_a) * sum sin^2(b - mu_b))."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    assert a.size == b.size
    mu_a = np.arctan2(np.sin(a).sum(), np.cos(a).sum())
    mu_b = np.arctan2(np.sin(b).sum(), np.cos(b).sum())
    sa, sb = np.sin(a - mu_a), np.sin(b - mu_b)
    return float((sa * sb).sum() / np.sqrt((sa * sa).sum() * (sb * sb).sum()))


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def measure_correlations(*args):
    """Both reference signatures:
      measure_correlations(path_to_transformations, r_pred, t_pred)   clustering_mnist.py / clustering_particles.py:
          the .npy file holds one row (rotation, tx, ty) per image;
      measure_correlations(r_gt, t_gt, r_pred, t_pred)                clustering_dsprites.py.
    Returns (r_corr, [x_corr, y_corr]): circular correlation of the rotation, Pearson correlation of each translation
    axis.  (The dsprites reference returns an undefined name here; this returns the list it computed.)"""
    if len(args) == 3:
        tr = np.load(args[0])
        r_gt, t_gt = tr[:, 0].reshape(tr.shape[0], 1), tr[:, 1:].reshape(tr.shape[0], 2)
        r_pred, t_pred = args[1], args[2]
    elif len(args) == 4:
        r_gt, t_gt, r_pred, t_pred = args
    else:
        raise TypeError('measure_correlations(path, r_pred, t_pred) or measure_correlations(r_gt, t_gt, r_pred, t_pred)')
    r_gt, t_gt, r_pred, t_pred = _np(r_gt), _np(t_gt), _np(r_pred), _np(t_pred)
    r_corr = circcorrcoef(r_gt, r_pred)
    x_corr = np.corrcoef(t_gt[:, 0], t_pred[:, 0])[0][1]
    y_corr = np.corrcoef(t_gt[:, 1], t_pred[:, 1])[0][1]
    return r_corr, [x_corr, y_corr]
