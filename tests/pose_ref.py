"""fp64 numpy restatement of the pose refinement of include/tvae_cluster.h (a plain helper module, used by
test_refine_cpu.py and test_refine_gpu.py), built on align_ref.sample: the extended templates, the tables num / pp / yy,
the scores, the selection rule and the pose update.

What the definition fixes in fp32 is taken in fp32 here as well: theta_a = theta + (float)a * dtheta (two roundings), the
factor t_scale as the fp32 value the kernel gets, and the pose update.  Everything else is fp64 on those values."""
import numpy as np

import align_ref
import frc_ref

F32 = np.float32


def angles(theta, A, dtheta):
    """-> fp32 [N][NA]: theta + (float)a * dtheta, the product and the sum each rounded to fp32."""
    th = np.asarray(theta, dtype=F32).reshape(-1, 1)
    a = np.arange(-A, A + 1, dtype=F32)[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        return (th + (a * F32(dtheta)).astype(F32)).astype(F32)


def mask_at(d, radius, edge):
    """The mask of frc_ref.mask at d pixels from the centre (radius and edge as the fp32 values the kernel gets)."""
    if radius is None or not float(F32(radius)) > 0:
        return np.ones_like(d)
    r, e = float(F32(radius)), float(F32(edge))
    out = np.where(d <= r, 1.0, 0.0)
    soft = (d > r) & (d < r + e)
    if e > 0:
        out = np.where(soft, 0.5 * (1 + np.cos(np.pi * (d - r) / np.where(soft, e, 1.0))), out)
    return out


def template_positions(n, S, theta_a, dx, t_scale):
    """theta_a [M] (any float), dx [M][2] -> (col, row, d) [M][ne][ne] fp64 on the extended grid r, q = -S .. n - 1 + S: where the
    pixel reads the reference, and its distance from the canonical centre in pixels."""
    th = np.asarray(theta_a, dtype=np.float64).reshape(-1)
    dx = np.asarray(dx, dtype=np.float64).reshape(-1, 2)
    t = float(F32(t_scale))
    g = np.arange(-S, n + S, dtype=np.float64)
    x0 = (2 * g / (n - 1) - 1)[None, None, :]
    x1 = (1 - 2 * g / (n - 1))[None, :, None]
    with np.errstate(invalid='ignore', over='ignore'):
        c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
        v0 = x0 - t * dx[:, 0, None, None]
        v1 = x1 - t * dx[:, 1, None, None]
        u0 = v0 * c - v1 * s
        u1 = v0 * s + v1 * c
        return (u0 + 1) * (n - 1) / 2, (1 - u1) * (n - 1) / 2, np.sqrt(u0 * u0 + u1 * u1) * (n - 1) / 2


def templates(refs, cls, theta, dx, t_scale, A, dtheta, S, mask_radius=None, mask_edge=0.0):
    """-> T [N][NA][C][ne][ne] fp64 (zeros for an image whose class is outside [0, K))."""
    refs = np.asarray(refs, dtype=np.float64)
    K, C, n, _ = refs.shape
    cls = np.asarray(cls).astype(np.int64)
    N, NA, ne = cls.size, 2 * A + 1, n + 2 * S
    th = angles(theta, A, dtheta)
    T = np.zeros((N, NA, C, ne, ne))
    ok = np.flatnonzero((cls >= 0) & (cls < K))
    if ok.size == 0:
        return T
    pad = np.zeros((ok.size, C, ne, ne))                     # the reference on the extended grid's index range: align_ref.sample
    pad[:, :, :n, :n] = refs[cls[ok]]                        # takes positions on the grid of the image it samples
    dxs = np.asarray(dx, dtype=np.float64).reshape(-1, 2)[ok]
    for ai in range(NA):
        col, row, d = template_positions(n, S, th[ok, ai], dxs, t_scale)
        with np.errstate(invalid='ignore'):
            inside = (col > -1) & (col < n) & (row > -1) & (row < n)
        # outside (-1, n) of the TRUE frame is an exact 0; inside it the padded plane's extra zeros are the zero border
        col_s, row_s = np.where(inside, col, -5.0), np.where(inside, row, -5.0)
        smp = align_ref.sample(pad, col_s, row_s)
        m = np.where(inside, mask_at(np.where(inside, d, 0.0), mask_radius, mask_edge), 0.0)
        T[ok, ai] = smp * m[:, None]
    return T


def tables(Y, T, S):
    """Y [N][C][n][n], T [N][NA][C][ne][ne] -> (num, pp [N][NA][NS][NS], yy [N]) in fp64: P(r, q) = T[r - sy][q - sx]."""
    Y = np.asarray(Y, dtype=np.float64)
    N, C, n, _ = Y.shape
    NA, NS = T.shape[1], 2 * S + 1
    num, pp = np.zeros((N, NA, NS, NS)), np.zeros((N, NA, NS, NS))
    for syi in range(NS):
        for sxi in range(NS):
            # extended index of T[r - sy][q - sx] for r = 0: S - sy = 2S - syi
            P = T[:, :, :, 2 * S - syi:2 * S - syi + n, 2 * S - sxi:2 * S - sxi + n]
            num[:, :, syi, sxi] = (P * Y[:, None]).sum(axis=(2, 3, 4))
            pp[:, :, syi, sxi] = (P * P).sum(axis=(2, 3, 4))
    return num, pp, (Y * Y).sum(axis=(1, 2, 3))


def scores(num, pp, yy):
    """fp64 tables (or the kernel's fp32 ones) -> fp32 scores [N][NA][NS][NS]: num / sqrt(pp yy) in fp64, rounded once; 0 where
    pp or yy is 0."""
    num, pp = np.asarray(num, dtype=np.float64), np.asarray(pp, dtype=np.float64)
    yy = np.asarray(yy, dtype=np.float64).reshape(-1, 1, 1, 1)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        zero = (pp == 0) | (yy == 0)
        den = np.sqrt(pp * yy)
        return np.where(zero, 0.0, num / np.where(zero, 1.0, den)).astype(F32)


def select(score, cls, K):
    """The selection rule on fp32 scores [N][NA][NS][NS] -> (best int [N][3] = (a, sy, sx), out fp32 [N][2] = (centre, best))."""
    score = np.asarray(score, dtype=F32)
    N, NA, NS, _ = score.shape
    A, S = NA // 2, NS // 2
    best, out = np.zeros((N, 3), dtype=np.int64), np.zeros((N, 2), dtype=F32)
    cls = np.asarray(cls).astype(np.int64)
    for i in range(N):
        if not 0 <= cls[i] < K:
            continue
        flat = score[i].reshape(-1)
        centre = flat[(A * NS + S) * NS + S]
        bi = (A * NS + S) * NS + S
        any_finite = bool(np.isfinite(centre))
        bv = centre if any_finite else F32(-np.inf)
        for e in range(flat.size):
            v = flat[e]
            if np.isfinite(v) and v > bv:
                bv, bi, any_finite = v, e, True
        if any_finite:
            out[i] = (centre if np.isfinite(centre) else F32(-np.inf), bv)
        best[i] = (bi // (NS * NS) - A, (bi // NS) % NS - S, bi % NS - S)
    return best, out


def update_pose(theta, dx, best, n, t_scale, dtheta):
    """fp32, as the header fixes it: a part of the pose whose index is 0 is copied bit for bit."""
    theta = np.asarray(theta, dtype=F32).reshape(-1)
    dx = np.asarray(dx, dtype=F32).reshape(-1, 2)
    best = np.asarray(best)
    a, sy, sx = best[:, 0], best[:, 1], best[:, 2]
    t, den = F32(t_scale), F32(n - 1)
    with np.errstate(invalid='ignore', over='ignore'):
        th_new = (theta + (a.astype(F32) * F32(dtheta)).astype(F32)).astype(F32)
        d0 = (dx[:, 0] + (((2 * sx).astype(F32) / den).astype(F32) / t).astype(F32)).astype(F32)
        d1 = (dx[:, 1] + (((-2 * sy).astype(F32) / den).astype(F32) / t).astype(F32)).astype(F32)
    th_out = np.where(a == 0, theta.view(np.int32), th_new.view(np.int32)).astype(np.int32).view(F32)
    dx_out = np.stack([np.where(sx == 0, dx[:, 0].view(np.int32), d0.view(np.int32)),
                       np.where(sy == 0, dx[:, 1].view(np.int32), d1.view(np.int32))], 1).astype(np.int32).view(F32)
    return th_out, dx_out


def refine(Y, theta, dx, cls, refs, t_scale, A, dtheta, S, mask_radius=None, mask_edge=0.0):
    """The whole definition -> dict(T, num, pp, yy, score, best, out, theta, dx)."""
    refs = np.asarray(refs)
    K, n = refs.shape[0], refs.shape[-1]
    T = templates(refs, cls, theta, dx, t_scale, A, dtheta, S, mask_radius, mask_edge)
    num, pp, yy = tables(Y, T, S)
    skipped = ~((np.asarray(cls) >= 0) & (np.asarray(cls) < K))
    yy = np.where(skipped, 0.0, yy)                          # a skipped image's rows of the tables are zeros
    sc = scores(num, pp, yy)
    best, out = select(sc, cls, K)
    th, d = update_pose(theta, dx, best, n, t_scale, dtheta)
    return dict(T=T, num=num, pp=pp, yy=yy, score=sc, best=best, out=out, theta=th, dx=d)


def render(refs, cls, theta, dx, t_scale):
    """Images that show refs[cls] at the poses (theta, dx): the template of the angle itself without shifts -> [N][C][n][n]."""
    return templates(refs, cls, theta, dx, t_scale, 0, 0.0, 0)[:, 0]


def smooth_refs(n, K, C=1, seed=0):
    """[K][C][n][n] fp32: sums of a few Gaussians, off-centre, without rotational symmetry, small at the border of the frame."""
    rng = np.random.default_rng(seed)
    g = np.arange(n) - (n - 1) / 2
    jj, ii = np.meshgrid(g, g)
    refs = np.zeros((K, C, n, n))
    for k in range(K):
        for ch in range(C):
            for _ in range(4):
                ci, cj = rng.uniform(-0.22, 0.22, 2) * n
                sig = rng.uniform(0.05, 0.09) * n
                refs[k, ch] += rng.uniform(0.5, 1.5) * np.exp(-((ii - ci) ** 2 + (jj - cj) ** 2) / (2 * sig * sig))
    return refs.astype(F32)


PLANTED = dict(n=32, K=3, N=24, A=3, S=2, dtheta=0.05, t=1.0)


def planted(seed=7, **over):
    """Images rendered from smooth references at planted poses that lie ON the candidate grid of a perturbed start: image i shows
    refs[cls[i]] at (theta_true, dx_true), and the start is theta_true - a dtheta and dx_true - (2 sx, -2 sy) / ((n - 1) t) for a
    planted candidate (a, sy, sx) drawn over the whole grid, the corners and the centre among them.
    -> dict(Y, refs, cls, theta, dx (the start, fp32), want [N][3], theta_true, dx_true, and the geometry)."""
    p = dict(PLANTED, **over)
    n, K, N, A, S, t = p['n'], p['K'], p['N'], p['A'], p['S'], p['t']
    rng = np.random.default_rng(seed)
    refs = smooth_refs(n, K, seed=seed + 1)
    cls = rng.integers(0, K, N)
    want = np.stack([rng.integers(-A, A + 1, N), rng.integers(-S, S + 1, N), rng.integers(-S, S + 1, N)], 1)
    want[0], want[1], want[2], want[3] = (0, 0, 0), (A, S, S), (-A, -S, -S), (A, -S, S)
    theta_true = rng.uniform(-np.pi, np.pi, N).astype(F32)
    dx_true = (rng.uniform(-0.12, 0.12, (N, 2)) / t).astype(F32)
    theta = (theta_true - (want[:, 0].astype(F32) * F32(p['dtheta'])).astype(F32)).astype(F32)
    shift = np.stack([2 * want[:, 2], -2 * want[:, 1]], 1).astype(F32) / F32(n - 1) / F32(t)
    dx = (dx_true - shift.astype(F32)).astype(F32)
    Y = render(refs, cls, theta_true, dx_true, t).astype(F32)
    return dict(p, Y=Y, refs=refs, cls=cls, theta=theta, dx=dx, want=want, theta_true=theta_true, dx_true=dx_true)


def cross_half_labels(labels, n_clusters):
    """The reference index of every image when each is scored against the half-set average it is NOT in, with the 2K references
    ordered [half 0 of class 0 .. K - 1, half 1 of class 0 .. K - 1]: an image at an even position of its class (half 0) gets
    K + k, one at an odd position k; labels outside [0, K) get -1."""
    labels = np.asarray(labels).astype(np.int64)
    order, seg, _ = align_ref.segments(labels, n_clusters)
    out = np.full(labels.size, -1, dtype=np.int64)
    for k, (even, odd) in enumerate(frc_ref.half_lists(order, seg, labels.size)):
        out[even] = n_clusters + k
        out[odd] = k
    return out
