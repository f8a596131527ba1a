"""fp64 numpy restatement of the aligned-image definition of include/tvae_cluster.h (a plain helper module, used by
test_align_cpu.py and test_align_gpu.py).

Coordinates as tvae.tables.image_coords: x0 = linspace(-1, 1, n) along columns, x1 = linspace(1, -1, n) along rows.  The
aligned image A_i at the canonical grid point u = (u0, u1) reads image i at
    x = (u0 c + u1 s + t dx0,  -u0 s + u1 c + t dx1),   col = (x0 + 1) (n - 1) / 2,   row = (1 - x1) (n - 1) / 2
bilinearly over the taps floor and floor + 1; a tap outside [0, n - 1] is 0 and a position that is not inside (-1, n) on
both axes (NaN included) gives exactly 0."""
import numpy as np


def positions(n, theta, dx, t_scale):
    """-> (col, row) [N][n][n] fp64: where the canonical pixel (i, j) reads its image."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    dx = np.asarray(dx, dtype=np.float64).reshape(-1, 2)
    t = float(t_scale)
    u0 = np.linspace(-1, 1, n)[None, None, :]
    u1 = np.linspace(1, -1, n)[None, :, None]
    with np.errstate(invalid='ignore', over='ignore'):
        c, s = np.cos(theta)[:, None, None], np.sin(theta)[:, None, None]
        x0 = u0 * c + u1 * s + t * dx[:, 0, None, None]
        x1 = -u0 * s + u1 * c + t * dx[:, 1, None, None]
        return (x0 + 1) * (n - 1) / 2, (1 - x1) * (n - 1) / 2


def sample(images, col, row):
    """images [N][C][n][n], col / row [N][n][n] -> [N][C][n][n] fp64 bilinear samples with a zero border."""
    Y = np.asarray(images, dtype=np.float64)
    N, C, n, _ = Y.shape
    with np.errstate(invalid='ignore'):
        inside = (col > -1) & (col < n) & (row > -1) & (row < n)          # False for NaN
    col, row = np.where(inside, col, 0.0), np.where(inside, row, 0.0)
    c0, r0 = np.floor(col).astype(np.int64), np.floor(row).astype(np.int64)
    wc, wr = (col - c0)[:, None], (row - r0)[:, None]
    P = np.zeros((N, C, n + 2, n + 2))                                    # the zero border, taps -1 .. n
    P[:, :, 1:-1, 1:-1] = Y
    ii = np.arange(N)[:, None, None]

    def tap(r, c):
        return np.moveaxis(P[ii, :, r + 1, c + 1], -1, 1)

    top = (1 - wc) * tap(r0, c0) + wc * tap(r0, c0 + 1)
    bot = (1 - wc) * tap(r0 + 1, c0) + wc * tap(r0 + 1, c0 + 1)
    return np.where(inside[:, None], (1 - wr) * top + wr * bot, 0.0)


def align_stack(images, theta, dx, t_scale=1.0):
    n = np.asarray(images).shape[-1]
    col, row = positions(n, theta, dx, t_scale)
    return sample(images, col, row)


def segments(labels, n_clusters):
    """-> (order, seg, counts) as tvae.align.segments defines them."""
    lab = np.asarray(labels).astype(np.int64)
    key = np.where((lab >= 0) & (lab < n_clusters), lab, n_clusters)
    order = np.argsort(key, kind='stable')
    counts = np.bincount(key, minlength=n_clusters + 1)[:n_clusters]
    return order, np.concatenate([[0], np.cumsum(counts)]), counts


def class_averages(aligned, order, seg, N=None):
    """Per-class mean of the aligned images [N][C][n][n] over order[seg[k]:seg[k + 1]]; entries of `order` outside
    [0, N) are skipped and do not count.  -> (avg [K][C][n][n] fp64, counts [K])."""
    A = np.asarray(aligned, dtype=np.float64)
    N = A.shape[0] if N is None else N
    K = len(seg) - 1
    avg, counts = np.zeros((K,) + A.shape[1:]), np.zeros(K, dtype=np.int64)
    for k in range(K):
        m = np.asarray(order[seg[k]:seg[k + 1]], dtype=np.int64)
        m = m[(m >= 0) & (m < N)]
        counts[k] = m.size
        if m.size:
            avg[k] = A[m].sum(0) / m.size
    return avg, counts
