"""fp64 numpy restatement of the eigenimage definitions of include/tvae_cluster.h (a plain helper module, used by
test_eigen_cpu.py and test_eigen_gpu.py), built on align_ref: the mask, the masked residuals d = m (A - mean), project,
backproject, the subspace iteration of tvae.eigen in fp64, and the planted case both test files share.

What the definition fixes in fp32 is taken in fp32 here as well: the mask is evaluated in fp64 and rounded to fp32 once, the
mean is the fp32 array the kernel gets.  Everything else is fp64 on those values."""
import numpy as np

import align_ref
import pose_ref

F32 = np.float32
EPS = 2.0 ** -24


def mask(n, radius=None, edge=0.0):
    """-> [n][n] fp64 holding fp32 values: the mask of tvae_class_frc at the canonical pixels, 1 everywhere for radius <= 0."""
    c = 0.5 * (n - 1)
    i = np.arange(n, dtype=np.float64)
    d = np.sqrt((i[:, None] - c) ** 2 + (i[None, :] - c) ** 2)
    return pose_ref.mask_at(d, radius, edge).astype(F32).astype(np.float64)


def members(order, seg, k, N):
    """-> (positions q, image indices) of the valid members of class k, ascending position; seg as given (monotone)."""
    q = np.arange(seg[k], seg[k + 1], dtype=np.int64)
    ids = np.asarray(order, dtype=np.int64)[q]
    ok = (ids >= 0) & (ids < N)
    return q[ok], ids[ok]


def residuals(aligned, mean, m, ids, k):
    """The rows of R_k: d = m * (A - mean[k]) of the images `ids`, [len(ids)][C][n][n] fp64."""
    A = np.asarray(aligned, dtype=np.float64)
    return m[None, None] * (A[ids] - np.asarray(mean, dtype=np.float64)[k][None])


def project(aligned, mean, V, order, seg, m):
    """-> (coef [N][J], norm2 [N]) fp64 by position in `order`; zeros for skipped entries and positions in no class."""
    N, K, J = aligned.shape[0], len(seg) - 1, V.shape[1]
    coef, norm2 = np.zeros((N, J)), np.zeros(N)
    for k in range(K):
        q, ids = members(order, seg, k, N)
        if q.size:
            D = residuals(aligned, mean, m, ids, k).reshape(q.size, -1)
            coef[q] = D @ np.asarray(V[k], dtype=np.float64).reshape(J, -1).T
            norm2[q] = (D * D).sum(1)
    return coef, norm2


def backproject(aligned, mean, coef, order, seg, m):
    """-> (W [K][J][C][n][n] fp64, counts [K])."""
    N, K, J = aligned.shape[0], len(seg) - 1, coef.shape[1]
    W, counts = np.zeros((K, J) + aligned.shape[1:]), np.zeros(K, dtype=np.int64)
    for k in range(K):
        q, ids = members(order, seg, k, N)
        counts[k] = q.size
        if q.size:
            D = residuals(aligned, mean, m, ids, k).reshape(q.size, -1)
            W[k] = (np.asarray(coef, dtype=np.float64)[q].T @ D).reshape(W[k].shape)
    return W, counts


def orthonormalise(W, floor=2.0 ** -40):
    """W [L][P] -> (Q [L][P], rank): the Gram-based step of tvae.eigen.orthonormalise for one class."""
    Q, rank = np.asarray(W, dtype=np.float64), 0
    for _ in range(2):
        e, U = np.linalg.eigh(Q @ Q.T)
        e, U = e[::-1], U[:, ::-1]
        keep = (e > e[0] * floor) & (e > 0)
        scale = np.where(keep, 1.0 / np.sqrt(np.where(keep, e, 1.0)), 0.0)
        Q = (U * scale[None, :]).T @ Q
        rank = int(keep.sum())
    return Q, rank


def subspace_iteration(R, components, oversample, power_iterations, V0):
    """The algorithm of tvae.eigen.class_eigenimages for one class on an explicit residual matrix R [m][P], fp64 throughout:
    -> (eigenvalues [J], eigenvectors [J][P], coordinates [m][J])."""
    m = R.shape[0]
    J, V = components, np.asarray(V0, dtype=np.float64)
    for _ in range(power_iterations + 1):
        V, rank = orthonormalise((R @ V.T).T @ R)                      # R^T R V, rows as vectors
    c = R @ V.T
    lam, vec, y = np.zeros(V.shape[0]), np.zeros_like(V), np.zeros_like(c)
    if m >= 2 and rank > 0:
        e, U = np.linalg.eigh((c.T @ c)[:rank, :rank] / (m - 1))
        U = U[:, ::-1]
        lam[:rank] = np.maximum(e[::-1], 0.0)
        vec[:rank] = U.T @ V[:rank]
        y[:, :rank] = c[:, :rank] @ U
    return lam[:J], vec[:J], y[:, :J]


def svd_reference(R):
    """-> (eigenvalues [r] descending, eigenvectors [r][P], coordinates [m][r]) of R^T R / (m - 1) from the SVD of R."""
    U, s, Vt = np.linalg.svd(R, full_matrices=False)
    return s * s / (R.shape[0] - 1), Vt, U * s[None, :]


def chain(n, C):
    """gamma of tvae_class_project: the longest chain of additions an output passes through, C ceil(n n / 256) per thread
    and the 8 levels of the tree over 256 threads."""
    return C * ((n * n + 255) // 256) + 8


# ---- the planted case --------------------------------------------------------------------------------------------------------
PLANTED_SIGMA = (1.0, 0.5, 0.25)          # three planted components, sigma halving
PLANTED_NOISE = 1e-5
PLANTED_J = 4
PLANTED_ORDERS = ((0, 0), (2, 0), (0, 3))
PLANTED_WIDTH = 0.25                      # coordinate units: an eighth of the side
HERMITE = (lambda z: 1 + 0 * z, lambda z: z, lambda z: z * z - 1, lambda z: z ** 3 - 3 * z)      # He_0 .. He_3


def planted_modes(u0, u1, n):
    """mu and E_0 .. E_2 at the canonical coordinates (u0, u1) (coordinate units): the Hermite functions
    He_a(x) He_b(y) exp(-(x^2 + y^2) / 4), x and y in units of PLANTED_WIDTH, of the orders PLANTED_ORDERS in their natural
    normalisation (squared norm a! b!: orthogonal, NOT of equal norm -- the higher orders carry more, which keeps the third
    component's eigenvalue above a thousand times the tolerance that the sampling bound of all three allows); mu is a
    twentieth of the order (0, 0).  Smooth, and a few percent of their peak at the frame's edge.  The shapes and the width
    are the best of a scan over the orders up to 3 and widths 0.2 .. 0.3 for the ratio of the eigenvalue tolerance to the
    third eigenvalue (test_eigen_cpu.py)."""
    x, y = u0 / PLANTED_WIDTH, u1 / PLANTED_WIDTH
    g = np.exp(-0.25 * (x * x + y * y))
    return 0.05 * g, [HERMITE[a](x) * HERMITE[b](y) * g for a, b in PLANTED_ORDERS]


def planted(n, C, m, seed, t=1.0):
    """One class of m particles: canonical images mu + sum_j s_ij sigma_j E_j rendered into each particle's frame in fp64 at a
    random theta and |dx| <= 2 pixels (the model's convention, y_i(x) = T_i((x - t dx) R(theta))), plus white noise of
    PLANTED_NOISE; channel c carries the canonical image times (-1)^c (channels
    that differ, all at full amplitude).  -> dict with Y fp32 [m][C][n][n], theta, dx fp32
    (dx divided by t, as the encoder would report it), labels, and the scores s [m][3]."""
    rng = np.random.default_rng(seed)
    theta = rng.uniform(-np.pi, np.pi, m)
    h = 2.0 / (n - 1)
    dx = rng.uniform(-2 * h, 2 * h, (m, 2))
    s = rng.standard_normal((m, 3))
    x0 = np.linspace(-1, 1, n)[None, None, :] - dx[:, 0, None, None]
    x1 = np.linspace(1, -1, n)[None, :, None] - dx[:, 1, None, None]
    c, sn = np.cos(theta)[:, None, None], np.sin(theta)[:, None, None]
    u0, u1 = x0 * c - x1 * sn, x0 * sn + x1 * c                        # u = (x - t dx) R(theta), R = [[c, s], [-s, c]]
    mu, E = planted_modes(u0, u1, n)
    T = mu + sum(s[:, j, None, None] * PLANTED_SIGMA[j] * E[j] for j in range(3))
    Y = np.stack([T * (-1.0) ** ch for ch in range(C)], 1) + PLANTED_NOISE * rng.standard_normal((m, C, n, n))
    return dict(n=n, C=C, m=m, t=t, Y=Y.astype(F32), theta=theta.astype(F32), dx=(dx / t).astype(F32),
                labels=np.zeros(m, dtype=np.int64), scores=s)


PLANTED_M = 120
PLANTED_PASSES = 3                        # power_iterations = 2: three project / backproject passes


def planted_reference(n, C, image_bounds):
    """The planted class of one geometry with its fp64 reference and the bounds the end-to-end tests use (computed once by the
    caller, never modified): `image_bounds` is test_align_gpu.image_bounds.  The mean handed to the code under test is the fp64
    mean of the aligned reference images rounded to fp32; R is the reference residual matrix against exactly that array under
    the soft mask ((n - 1) / 2 - 2, edge 2), and lam / vec / coords its fp64 decomposition.
        B   = m b_q + 3 2^-24 |d|                                  per element: what a computed residual may be off by
        dS  = 2 |R|_F |B|_F + |B|_F^2 + 2 gamma 2^-24 |R|_F^2      perturbation of R^T R as the iteration sees it
        lam_tol = 2 dS / (m - 1) (Weyl),   sine_j = 2 dS / ((m - 1) gap_j) (Davis-Kahan)."""
    t = 1.0 if C == 1 else 0.1
    p = planted(n, C, PLANTED_M, 100 * n + C, t)
    m = p['m']
    A = align_ref.align_stack(p['Y'], p['theta'], p['dx'], float(F32(t)))
    mean = A.mean(0).astype(F32)[None]
    radius, edge = (n - 1) / 2 - 2, 2.0
    mk = mask(n, radius, edge)
    R = residuals(A, mean, mk, np.arange(m), 0).reshape(m, -1)
    lam, vec, coords = svd_reference(R)
    b = image_bounds(p['Y'], p['dx'], t)
    B = (mk[None, None] * b[:, None, None, None] * np.ones((1, C, 1, 1))).reshape(m, -1) + 3 * EPS * np.abs(R)
    nR, nB = np.linalg.norm(R), np.linalg.norm(B)
    dS = 2 * nR * nB + nB ** 2 + 2 * chain(n, C) * EPS * nR ** 2
    gap = np.array([min(lam[j - 1] - lam[j] if j else np.inf, lam[j] - lam[j + 1]) for j in range(3)])
    out = dict(p, aligned=A, mean=mean, radius=radius, edge=edge, mask=mk, R=R, B=B, lam=lam, vec=vec, coords=coords, dS=dS,
               lam_tol=2 * dS / (m - 1), sine=2 * dS / ((m - 1) * gap), gap=gap)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
