"""fp64 numpy restatement of the class statistics of include/tvae_cluster.h (a plain helper module, used by
test_class_stats_cpu.py and test_class_stats_gpu.py): the half-set averages and the variance of a class from the aligned
images of tests/align_ref.py, and the Fourier ring correlation with np.fft.fft2 and the integer ring rule.

Halves: position q of a member counts from the class's first position in `order`, a skipped entry keeps its position;
half 0 takes the even q, half 1 the odd q.  Variance: the sample variance of the members' aligned images (two-pass form
here; the kernel uses the sum-of-squares form).  Ring of (ky, kx), signed frequencies in fftfreq order: the integer r with
(2r - 1)^2 <= 4 (ky^2 + kx^2) < (2r + 1)^2, i.e. the radius rounded half up; rings 0 .. n // 2 are kept."""
import math

import numpy as np

EPS = 2.0 ** -24


# ---- halves and variance ---------------------------------------------------------------------------------------------------
def half_lists(order, seg, N):
    """-> [K][2] arrays of image indices: the valid members of class k at even / odd positions, in ascending position."""
    out = []
    for k in range(len(seg) - 1):
        m = np.asarray(order[seg[k]:seg[k + 1]], dtype=np.int64)
        q = np.arange(m.size)
        ok = (m >= 0) & (m < N)
        out.append([m[ok & (q % 2 == 0)], m[ok & (q % 2 == 1)]])
    return out


def as_segments(lists):
    """A list of index arrays as (order, seg) of that many classes."""
    order = np.concatenate([np.asarray(m, dtype=np.int64) for m in lists] + [np.zeros(0, dtype=np.int64)])
    return order, np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int64)


def class_halves(aligned, order, seg, N=None):
    """-> (avg [K][C][n][n], halves [2][K][C][n][n], var [K][C][n][n], counts [K][2]) in fp64 / int64."""
    A = np.asarray(aligned, dtype=np.float64)
    N = A.shape[0] if N is None else N
    K = len(seg) - 1
    avg, var = np.zeros((K,) + A.shape[1:]), np.zeros((K,) + A.shape[1:])
    halves, counts = np.zeros((2, K) + A.shape[1:]), np.zeros((K, 2), dtype=np.int64)
    for k, pair in enumerate(half_lists(order, seg, N)):
        for h, m in enumerate(pair):
            counts[k, h] = m.size
            if m.size:
                halves[h, k] = A[m].sum(0) / m.size
        both = np.concatenate(pair)
        if both.size:
            avg[k] = A[both].sum(0) / both.size
        if both.size >= 2:
            var[k] = ((A[both] - avg[k]) ** 2).sum(0) / (both.size - 1)
    return avg, halves, var, counts


# ---- ring correlation ------------------------------------------------------------------------------------------------------
def signed_freq(n):
    """fftfreq order: 0, 1, ..., then the negative ones (index n // 2 of an even n is -n / 2)."""
    idx = np.arange(n)
    return np.where(idx < (n + 1) // 2, idx, idx - n)


def ring_of(ky, kx):
    """The radius of the integer point rounded half up, in exact integer arithmetic: floor(sqrt(s) + 1/2) =
    (floor(sqrt(4 s)) + 1) // 2."""
    return (math.isqrt(4 * (int(ky) * int(ky) + int(kx) * int(kx))) + 1) // 2


def ring_index(n):
    """[n][n] ints, both axes in fftfreq order; entries above n // 2 are the dropped corners."""
    k = signed_freq(n)
    return np.array([[ring_of(ky, kx) for kx in k] for ky in k], dtype=np.int64)


def mask(n, radius, edge=0.0):
    """[n][n] fp64: 1 within `radius` of the centre ((n - 1) / 2, (n - 1) / 2), a raised cosine over `edge`, 0 beyond;
    radius <= 0 (or None): no mask.  radius and edge are taken as the fp32 values the kernel gets."""
    if radius is None or not float(np.float32(radius)) > 0:
        return np.ones((n, n))
    r, e = float(np.float32(radius)), float(np.float32(edge))
    c = (n - 1) / 2
    i, j = np.meshgrid(np.arange(n) - c, np.arange(n) - c, indexing='ij')
    d = np.sqrt(i * i + j * j)
    out = np.where(d <= r, 1.0, 0.0)
    soft = (d > r) & (d < r + e)
    if e > 0:
        out = np.where(soft, 0.5 * (1 + np.cos(np.pi * (d - r) / np.where(soft, e, 1.0))), out)
    return out


def ring_sums(Fa, Fb):
    """Fa, Fb [P][n][n] complex -> sums [P][R][3]: (sum Re(Fa conj Fb), sum |Fa|^2, sum |Fb|^2) per ring."""
    P, n, _ = Fa.shape
    R = n // 2 + 1
    ring = ring_index(n).reshape(-1)
    keep = ring < R
    terms = np.stack([(Fa * np.conj(Fb)).real, np.abs(Fa) ** 2, np.abs(Fb) ** 2], -1).reshape(P, n * n, 3)
    sums = np.zeros((P, R, 3))
    for p in range(P):
        for q in range(3):
            sums[p, :, q] = np.bincount(ring[keep], weights=terms[p, keep, q], minlength=R)
    return sums


def frc_from_sums(sums):
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        den = np.sqrt(s[..., 1] * s[..., 2])
        return np.where((s[..., 1] == 0) | (s[..., 2] == 0), 0.0, s[..., 0] / np.where(den == 0, 1.0, den))


def frc(a, b, radius=None, edge=0.0):
    """a, b [P][n][n] -> dict(frc [P][R], sums [P][R][3], Fa, Fb [P][n][n] complex, am, bm the masked planes)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = mask(a.shape[-1], radius, edge)
    am, bm = a * m, b * m
    Fa, Fb = np.fft.fft2(am), np.fft.fft2(bm)
    sums = ring_sums(Fa, Fb)
    return dict(frc=frc_from_sums(sums), sums=sums, Fa=Fa, Fb=Fb, am=am, bm=bm)


def frc_bounds(ref):
    """From the reference alone: a coefficient of the two-stage fp32 DFT is within B_a = (2 n + 16) 2^-24 sum |a m| of the
    exact one (n additions per stage, each relative to a partial sum of at most sum |a m|, the twiddles and the products),
    hence per coefficient |d(Fa conj Fb)| <= B_a |Fb| + B_b |Fa| + B_a B_b and |d |Fa|^2| <= 2 B_a |Fa| + B_a^2, summed
    over the ring.  -> [P][R][3]."""
    Fa, Fb = ref['Fa'], ref['Fb']
    P, n, _ = Fa.shape
    R = n // 2 + 1
    Ba = ((2 * n + 16) * EPS * np.abs(ref['am']).sum(axis=(1, 2)))[:, None, None]
    Bb = ((2 * n + 16) * EPS * np.abs(ref['bm']).sum(axis=(1, 2)))[:, None, None]
    fa, fb = np.abs(Fa), np.abs(Fb)
    terms = np.stack([Ba * fb + Bb * fa + Ba * Bb, 2 * Ba * fa + Ba * Ba, 2 * Bb * fb + Bb * Bb], -1).reshape(P, n * n, 3)
    ring = ring_index(n).reshape(-1)
    keep = ring < R
    out = np.zeros((P, R, 3))
    for p in range(P):
        for q in range(3):
            out[p, :, q] = np.bincount(ring[keep], weights=terms[p, keep, q], minlength=R)
    return out
