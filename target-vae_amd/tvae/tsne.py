"""t-SNE of the content latents on the GPU (the `TSNE(2, learning_rate=200.0, init='random')` step of the reference
clustering_*.py), with the repulsion computed EXACTLY.

The algorithm is sklearn's default TSNE -- sparse input similarities over the K = min(N - 1, int(3 * perplexity + 1))
nearest neighbours, per-row bisection on the entropy, P + P^T normalised, early exaggeration 12 for 250 iterations at
momentum 0.5 and then momentum 0.8, the gain rule of `_gradient_descent`, the convergence checks every 50 iterations --
with one deliberate difference: sklearn approximates the repulsive half of the gradient with a Barnes-Hut tree
(angle = 0.5); here sum_j q_ij^2 (y_i - y_j) and Z = sum q_ij run over ALL pairs, every iteration, on the HIP kernels of
libtvae_cluster.so (include/tvae_cluster.h: tvae_knn, tvae_tsne_repulsion, tvae_tsne_step, tvae_tsne_kl).  No N x N
matrix exists at any point, there are no float atomics (a run is bitwise reproducible under a seed) and the host
only synchronises at the convergence checks.  There is no CPU fallback for the kernels.

The bisection and the symmetrisation into CSR run once per embedding over N * K values; they are torch code that does
not care where its tensors live (conditional_probabilities and joint_probabilities also run on CPU tensors).
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from . import _cluster_lib as CL
from ._lib import TvaeHipError

TSNEResult = namedtuple('TSNEResult', 'embedding kl_divergence n_iter')
CSR = namedtuple('CSR', 'rowptr col val')          # int32 [N + 1], int32 [nnz], fp32 [nnz]

MAX_POINTS = 1 << 24
EXPLORATION_ITER = 250                # sklearn's _EXPLORATION_MAX_ITER
N_ITER_CHECK = 50                     # sklearn's _N_ITER_CHECK
N_ITER_WITHOUT_PROGRESS = 300
MIN_GRAD_NORM = 1e-7
BISECTION_STEPS = 100
PERPLEXITY_TOLERANCE = 1e-5
EPS64 = float(np.finfo(np.float64).eps)


def n_neighbors(N, perplexity):
    return min(N - 1, int(3.0 * perplexity + 1))


def _feature_major(X):
    N, d = X.shape
    ld = (N + 3) // 4 * 4
    Xt = torch.zeros(d, ld, dtype=torch.float32, device=X.device)
    Xt[:, :N] = X.t()
    return Xt, ld


def _check_points(X, what):
    if not (CL.is_f32(X, contiguous=False) and X.dim() == 2):
        raise TvaeHipError(f'{what}: X must be a CUDA fp32 [N][d] tensor (no CPU fallback)')
    N, d = X.shape
    if not (2 <= N <= MAX_POINTS and 1 <= d <= 256):
        raise TvaeHipError(f'{what}: N={N}, d={d} outside the supported range (2 <= N <= 2^24, 1 <= d <= 256)')
    return N, d


def knn(X, n_neighbors):
    """The n_neighbors nearest other points of every row of X (CUDA fp32 [N][d]) under the squared Euclidean distance,
    brute force on the GPU -> (idx int32 [N][K], d2 fp32 [N][K]), each row ascending by (d2, index)."""
    N, d = _check_points(X, 'knn')
    K = int(n_neighbors)
    if not (1 <= K <= 256 and K < N):
        raise TvaeHipError(f'knn: n_neighbors = {K} must be in [1, 256] and below N = {N}')
    if not bool(torch.isfinite(X).all()):
        raise TvaeHipError('knn: X holds NaN or Inf')
    Xt, ldx = _feature_major(X.contiguous())
    idx = torch.empty(N, K, dtype=torch.int32, device=X.device)
    d2 = torch.empty(N, K, dtype=torch.float32, device=X.device)
    CL.call('tvae_knn', Xt, ldx, idx, d2, N, d, K)
    return idx, d2


def conditional_probabilities(d2, perplexity=30.0):
    """Row-wise p_{j|i} over the K neighbour distances d2 [N][K] (squared), any device -> fp32 [N][K].

    sklearn's `_binary_search_perplexity`: beta = 1, up to 100 bisection steps on H(beta) - ln(perplexity) with tolerance
    1e-5, beta doubled (halved) while the upper (lower) bound is still infinite.  All rows advance together in fp64; a
    row that has met the tolerance is frozen."""
    if not (torch.is_tensor(d2) and d2.dim() == 2):
        raise TvaeHipError('conditional_probabilities: d2 must be an [N][K] tensor')
    D = d2.to(torch.float64)
    N = D.shape[0]
    target = math.log(perplexity)
    inf = float('inf')
    beta = torch.ones(N, 1, dtype=torch.float64, device=D.device)
    lo = torch.full_like(beta, -inf)
    hi = torch.full_like(beta, inf)
    done = torch.zeros(N, 1, dtype=torch.bool, device=D.device)
    P = torch.zeros_like(D)
    for step in range(BISECTION_STEPS):
        Pn = torch.exp(-D * beta)
        s = Pn.sum(1, keepdim=True)
        s = torch.where(s == 0, torch.full_like(s, 1e-8), s)
        Pn = Pn / s
        H = torch.log(s) + beta * (D * Pn).sum(1, keepdim=True)
        diff = H - target
        P = torch.where(done, P, Pn)
        done = done | (diff.abs() <= PERPLEXITY_TOLERANCE)
        up = diff > 0
        lo = torch.where(~done & up, beta, lo)
        hi = torch.where(~done & ~up, beta, hi)
        nb = torch.where(up, torch.where(hi == inf, beta * 2, (beta + hi) / 2),
                         torch.where(lo == -inf, beta / 2, (beta + lo) / 2))
        beta = torch.where(done, beta, nb)
        if step % 8 == 7 and bool(done.all()):
            break
    return P.to(torch.float32)


def joint_probabilities(idx, cond_p):
    """(P + P^T) / sum over the neighbour graph (idx [N][K], cond_p [N][K]; any device) -> CSR(rowptr, col, val) with
    ascending columns within a row.  An entry is the sum of at most two values, so it does not depend on any order;
    the matrix is exactly symmetric.  tvae_knn leaves idx = -1 where a row has fewer than K finite distances (finite but
    huge X whose squared distances overflow): such a graph is refused, an index outside [0, N) would land in another row."""
    N, K = idx.shape
    dev = idx.device
    if tuple(cond_p.shape) != (N, K):
        raise TvaeHipError(f'joint_probabilities: cond_p must be [{N}][{K}] like idx')
    if bool(((idx < 0) | (idx >= N)).any()):
        raise TvaeHipError('joint_probabilities: the neighbour graph holds indices outside [0, N) (tvae_knn marks a '
                           'neighbour it could not find, a non-finite distance, with -1)')
    rows = torch.arange(N, device=dev, dtype=torch.int64).unsqueeze(1).expand(N, K).reshape(-1)
    cols = idx.reshape(-1).to(torch.int64)
    v = cond_p.reshape(-1).to(torch.float64)
    key = torch.cat([rows * N + cols, cols * N + rows])
    key, order = torch.sort(key, stable=True)
    v2 = torch.cat([v, v])[order]
    nxt_same = torch.zeros_like(key, dtype=torch.bool)
    nxt_same[:-1] = key[1:] == key[:-1]
    first = torch.ones_like(nxt_same)
    first[1:] = ~nxt_same[:-1]
    partner = torch.zeros_like(v2)
    partner[:-1] = v2[1:]
    val = (v2 + torch.where(nxt_same, partner, torch.zeros_like(v2)))[first]
    ukey = key[first]
    val = val / torch.clamp(val.sum(), min=EPS64)
    r = ukey // N
    rowptr = torch.searchsorted(r, torch.arange(N + 1, device=dev, dtype=torch.int64))
    return CSR(rowptr.to(torch.int32), (ukey - r * N).to(torch.int32), val.to(torch.float32).contiguous())


class _State:
    """Device buffers of one embedding: the ping-pong Y, gains, update, the repulsion sums and the workspaces."""

    def __init__(self, N, dev):
        self.N, self.ld = N, (N + 3) // 4 * 4
        z = lambda: torch.zeros(2, self.ld, dtype=torch.float32, device=dev)    # noqa: E731
        self.Y = [z(), z()]
        self.gains, self.update, self.rep, self.grad = z(), z(), z(), z()
        self.gains.fill_(1.0)
        self.Z = torch.zeros(1, dtype=torch.float64, device=dev)
        self.kl = torch.zeros(1, dtype=torch.float64, device=dev)
        self.groups = CL.query('tvae_tsne_groups', N)
        self.ws_floats = CL.query('tvae_tsne_repulsion_ws_floats', N)
        if self.groups <= 0 or self.ws_floats <= 0:
            raise TvaeHipError(f'tsne: N={N} is not supported by libtvae_cluster.so')
        self.ws = CL.workspace(self.ws_floats, dev)
        self.gn2 = torch.zeros(self.groups, dtype=torch.float64, device=dev)
        self.klws = torch.zeros(self.groups, dtype=torch.float64, device=dev)

    def repulsion(self, cur):
        CL.call('tvae_tsne_repulsion', self.Y[cur], self.ld, self.rep, self.Z, self.ws, self.ws.numel(), self.N)

    def kl_of(self, P, cur):
        CL.call('tvae_tsne_kl', P.rowptr, P.col, P.val, P.val.numel(), self.Y[cur], self.ld, self.Z, self.kl, self.klws,
                self.groups, self.N)

    def step(self, P, cur, alpha, momentum, lr, grad=None):
        CL.call('tvae_tsne_step', P.rowptr, P.col, P.val, P.val.numel(), self.Y[cur], self.rep, self.Z, self.gains,
                self.update, self.Y[1 - cur], grad, self.gn2, self.ld, self.N, alpha, momentum, lr)


def _check_embedding(Y, P):
    if not (torch.is_tensor(Y) and Y.is_cuda and Y.dim() == 2 and Y.shape[1] == 2):
        raise TvaeHipError('tsne: the embedding must be a CUDA [N][2] tensor (no CPU fallback)')
    N = Y.shape[0]
    if not (2 <= N <= MAX_POINTS and P.rowptr.numel() == N + 1 and P.val.numel() >= 1 and P.col.numel() == P.val.numel()):
        raise TvaeHipError('tsne: the CSR matrix does not fit the embedding')
    return N


def gradient(Y, P, exaggeration=1.0):
    """The exact KL gradient at the embedding Y (CUDA [N][2]) for the joint probabilities P (CSR on the same device) ->
    (grad fp32 [N][2], Z, KL divergence): one repulsion, one step whose update is thrown away, one KL pass."""
    N = _check_embedding(Y, P)
    st = _State(N, Y.device)
    st.Y[0][:, :N] = Y.to(torch.float32).t()
    st.repulsion(0)
    st.kl_of(P, 0)
    st.step(P, 0, float(exaggeration), 0.0, 0.0, grad=st.grad)
    return st.grad[:, :N].t().contiguous(), float(st.Z), float(st.kl)


def _descend(st, P, cur, it0, it1, alpha, momentum, lr, patience):
    """sklearn's `_gradient_descent` from iteration it0 to it1 (exclusive) -> (cur, last iteration index).  The error that
    the progress rule watches is the KL divergence of the exaggerated P, alpha (KL + ln alpha), as in sklearn."""
    best_err, best_it, i = float('inf'), it0, it0
    for i in range(it0, it1):
        check = (i + 1) % N_ITER_CHECK == 0
        st.repulsion(cur)
        if check:
            st.kl_of(P, cur)
        st.step(P, cur, alpha, momentum, lr)
        cur = 1 - cur
        if check:
            host = torch.cat([st.kl, st.gn2]).cpu().numpy()               # the only synchronisation: one D2H copy
            err = alpha * (float(host[0]) + math.log(alpha))
            gnorm = math.sqrt(float(host[1:].sum()))
            if err < best_err:
                best_err, best_it = err, i
            elif i - best_it > patience:
                break
            if gnorm <= MIN_GRAD_NORM:
                break
    return cur, i


def tsne(X, perplexity=30.0, early_exaggeration=12.0, learning_rate=200.0, max_iter=1000, seed=None, init=None):
    """Embed the rows of X (CUDA fp32 [N][d]) in two dimensions.

    init: optional [N][2] starting embedding; otherwise 1e-4 * standard normal (fp32) from a torch.Generator seeded with
    `seed` (unseeded when None).  Returns TSNEResult(embedding CUDA fp32 [N][2], kl_divergence of that embedding against
    the un-exaggerated P, n_iter = iterations run)."""
    N, d = _check_points(X, 'tsne')
    if not perplexity < N:
        raise TvaeHipError(f'tsne: perplexity = {perplexity} must be less than N = {N}')
    if not (perplexity > 0 and early_exaggeration >= 1 and learning_rate > 0 and max_iter >= EXPLORATION_ITER):
        raise TvaeHipError('tsne: perplexity > 0, early_exaggeration >= 1, learning_rate > 0 and max_iter >= 250 are required')
    K = n_neighbors(N, perplexity)
    if K > 256:
        raise TvaeHipError(f'tsne: perplexity = {perplexity} needs {K} neighbours, the kernels keep at most 256')
    dev = X.device
    if init is not None:
        if not (torch.is_tensor(init) and tuple(init.shape) == (N, 2)):
            raise TvaeHipError(f'tsne: init must be [{N}][2]')
        Y0 = init.to(device=dev, dtype=torch.float32)
    else:
        g = torch.Generator(device=dev)
        if seed is None:
            g.seed()
        else:
            g.manual_seed(int(seed))
        Y0 = 1e-4 * torch.randn(N, 2, generator=g, device=dev, dtype=torch.float32)
    idx, d2 = knn(X, K)
    P = joint_probabilities(idx, conditional_probabilities(d2, perplexity))
    st = _State(N, dev)
    st.Y[0][:, :N] = Y0.t()
    cur, it = _descend(st, P, 0, 0, EXPLORATION_ITER, float(early_exaggeration), 0.5, float(learning_rate), EXPLORATION_ITER)
    if max_iter > it + 1:
        cur, it = _descend(st, P, cur, it + 1, int(max_iter), 1.0, 0.8, float(learning_rate), N_ITER_WITHOUT_PROGRESS)
    st.repulsion(cur)
    st.kl_of(P, cur)
    return TSNEResult(st.Y[cur][:, :N].t().contiguous(), float(st.kl), it + 1)
