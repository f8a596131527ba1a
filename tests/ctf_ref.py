"""fp64 numpy restatement of the CTF section of include/tvae_cluster.h (a plain helper module, used by test_ctf_cpu.py and
test_ctf_gpu.py): the transfer function from its five coefficients, the Fourier filter with a real half-spectrum plane, the
per-class power sums and the two CTF-corrected class averages on top of tests/align_ref.py.  Every function takes the
fp32 inputs converted to double.  `filter_f32` is the SAME four stages in float32 numpy (for the per-element limit of
test_ctf_gpu.py) and `filter_bound` the a-priori Frobenius bound derived there."""
import numpy as np

import align_ref

EPS = 2.0 ** -24


def signed(n):
    """ks(ky), ky = 0 .. n - 1: the signed frequencies in numpy's fftfreq order."""
    return np.rint(np.fft.fftfreq(n) * n).astype(np.int64)


def q_grid(n):
    """q[n][R] = (ks(ky)^2 + kx^2) / n^2 from the exact integer numerator."""
    R = n // 2 + 1
    num = signed(n)[:, None] ** 2 + np.arange(R)[None, :] ** 2
    return num.astype(np.float64) / float(n * n)


def H(coef, n, mode=0):
    """coef [N][5] -> H fp64 [N][n][R]; mode 1: the sign (-1 for H < 0, +1 for anything else)."""
    c = np.asarray(coef, dtype=np.float64).reshape(-1, 5)[:, :, None, None]
    q = q_grid(n)[None]
    t = c[:, 2] * q + c[:, 3] * q * q
    h = (c[:, 0] * np.sin(2 * np.pi * t) + c[:, 1] * np.cos(2 * np.pi * t)) * np.exp(-c[:, 4] * q)
    return np.where(h < 0, -1.0, 1.0) if mode == 1 else h


def weights(n):
    """w_kx [R]: 1 for kx = 0 and for the Nyquist column of an even n, 2 for every other one."""
    w = np.full(n // 2 + 1, 2.0)
    w[0] = 1.0
    if n % 2 == 0:
        w[-1] = 1.0
    return w


def full_plane(Hh, n):
    """[..][n][R] -> [..][n][n]: the half plane extended by H(-ky, -kx)."""
    Hh = np.asarray(Hh, dtype=np.float64)
    R = n // 2 + 1
    out = np.empty(Hh.shape[:-1] + (n,))
    out[..., :R] = Hh
    ky = (-np.arange(n)) % n
    for kx in range(R, n):
        out[..., kx] = Hh[..., ky, n - kx]
    return out


def filter(x, Hh):
    """x [..][n][n], Hh [..][n][R] (broadcast against each other) -> Re ifft2(fft2(x) * H) on the full plane, fp64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    return np.fft.ifft2(np.fft.fft2(x) * full_plane(Hh, n)).real


def twiddle_tables(n, dtype=np.float64):
    """C, S [n][n]: cos and sin of 2 pi ((a b) mod n) / n, the argument reduced in integers."""
    t = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    return np.cos(2 * np.pi * t / n).astype(dtype), np.sin(2 * np.pi * t / n).astype(dtype)


def filter_f32(x, Hh):
    """The four stages of the kernel in float32 numpy: x [B][n][n] fp32, Hh [B][n][R] or [n][R] fp32 -> [B][n][n] fp32."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[-1]
    R = n // 2 + 1
    C, S = twiddle_tables(n, np.float32)
    hw = np.asarray(Hh, dtype=np.float32) * weights(n).astype(np.float32)
    Gr, Gi = x @ C[:, :R], -(x @ S[:, :R])
    Fr, Fi = C @ Gr + S @ Gi, C @ Gi - S @ Gr
    Fr, Fi = Fr * hw, Fi * hw
    Pr, Pi = C @ Fr - S @ Fi, C @ Fi + S @ Fr
    return ((Pr @ C[:R, :] - Pi @ S[:R, :]) * np.float32(1.0 / (np.float32(n) * np.float32(n)))).astype(np.float32)


def filter_bound(x, Hh, c01=0.0):
    """The a-priori Frobenius bound [B] of test_ctf_gpu.py's docstring on |kernel - filter(x, Hh)| per plane; x [B][n][n],
    Hh [B][n][R] or [n][R] (fp64 values of what the kernel multiplies with), c01 = |c0| + |c1| per plane in coefficient
    mode ([B] or a scalar), 0 where the kernel reads the plane."""
    x = np.asarray(x, dtype=np.float64)
    B, n = x.shape[0], x.shape[-1]
    R = n // 2 + 1
    hw = np.broadcast_to(np.abs(np.asarray(Hh, dtype=np.float64)) * weights(n), (B, n, R))
    G = np.fft.fft(x, axis=-1)[..., :R]
    F = np.fft.fft(G, axis=-2)
    g1, g2, g2r = (n + 2) * EPS, (2 * n + 2) * EPS, (2 * R + 2) * EPS
    nx = np.sqrt((x ** 2).sum((1, 2)))
    gcol2 = (np.abs(G) ** 2).sum(1)                                        # [B][R]
    nFp = np.sqrt((np.abs(F) ** 2 * hw ** 2).sum((1, 2)))                 # |F'|
    nFw = np.sqrt((np.abs(F) ** 2 * weights(n) ** 2).sum((1, 2)))
    e1 = g1 * nx * np.sqrt((hw.max(1) ** 2).sum(1))
    e2 = np.sqrt(2) * g2 / np.sqrt(n) * np.sqrt((gcol2 * (hw ** 2).sum(1)).sum(1))
    em = EPS * nFp / n + 8 * EPS * np.asarray(c01, dtype=np.float64) * nFw / n
    e3 = np.sqrt(2) * g2 / np.sqrt(n) * nFp
    e4 = g2r * np.sqrt(R) * nFp / n
    ref = filter(x, Hh)
    return e1 + e2 + em + e3 + e4 + EPS * np.sqrt((ref ** 2).sum((1, 2)))


def power(coef, order, seg, n, N=None):
    """-> (D fp64 [K][n][R], counts [K]): the sums of H_i^2 over order[seg[k]:seg[k + 1]], entries outside [0, N) skipped;
    seg cleaned as the header states (running maximum, clamped to [0, N])."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 5)
    N = coef.shape[0] if N is None else N
    clean = np.minimum(np.maximum.accumulate(np.maximum(np.asarray(seg, dtype=np.int64), 0)), N)
    K = len(seg) - 1
    h2 = H(coef, n) ** 2
    D, counts = np.zeros((K, n, n // 2 + 1)), np.zeros(K, dtype=np.int64)
    for k in range(K):
        m = np.asarray(order[clean[k]:clean[k + 1]], dtype=np.int64)
        m = m[(m >= 0) & (m < N)]
        counts[k] = m.size
        for i in m:                                                        # ascending position
            D[k] += h2[i]
    return D, counts


def class_averages_ctf(images, theta, dx, labels, coef, n_clusters, t_scale=1.0, correct='wiener', tau=0.1):
    """-> (avg fp64 [K][C][n][n], counts [K], D [K][n][R]) as tvae.ctf.class_averages_ctf defines them."""
    Y = np.asarray(images, dtype=np.float64)
    N, C, n, _ = Y.shape
    order, seg, _ = align_ref.segments(labels, n_clusters)
    D, counts = power(coef, order, seg, n)
    Hh = H(coef, n, 1 if correct == 'flip' else 0)
    xf = filter(Y, Hh[:, None])
    mean, _ = align_ref.class_averages(align_ref.align_stack(xf, theta, dx, t_scale), order, seg)
    if correct == 'flip':
        return mean, counts, D
    G = 1.0 / (D / np.maximum(counts, 1)[:, None, None] + tau)
    return filter(mean, G[:, None]), counts, D
