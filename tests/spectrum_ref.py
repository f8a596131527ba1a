"""fp64 numpy restatement of the section "Radial spectra" of include/tvae_cluster.h (a plain helper module, used by
test_spectrum_cpu.py and test_spectrum_gpu.py): the window, the window-weighted mean, the transform, the integer ring rule
over the whole plane, the ring power and its normalisation, the group sums, the profile lookup in both interpolation modes
and the radial filter.  `power_f32` is stages 1 and 2 in float32 numpy, as ctf_ref.filter_f32 restates the filter, and
`power_bound` the a-priori bound derived in test_spectrum_gpu.py."""
import math

import numpy as np

import ctf_ref
import frc_ref

EPS = 2.0 ** -24


def rings(n):
    """Rr = 1 + ring(h, h), h = n // 2."""
    h = n // 2
    return 1 + frc_ref.ring_of(h, h)


def ring_index(n):
    """[n][n] ints, both axes in fftfreq order, corners included."""
    return frc_ref.ring_index(n)


def ring_counts(n):
    return np.bincount(ring_index(n).reshape(-1), minlength=rings(n)).astype(np.float64)


def window(n, radius, edge, background):
    """fp64 [n][n] holding the fp32 values of the window: m is the FRC's mask rounded to fp32 (the kernel's soft_mask returns
    a float), w = 1 - m in fp32 for the background."""
    if radius is None or not float(np.float32(radius)) > 0:
        return np.ones((n, n))
    m = frc_ref.mask(n, radius, edge).astype(np.float32)
    return (np.float32(1.0) - m if background else m).astype(np.float64)


def windowed(X, radius, edge, background, demean):
    """X [B][n][n] -> (y fp64 [B][n][n] = (x - mu) w exactly, mu [B])."""
    x = np.asarray(X, dtype=np.float64)
    w = window(x.shape[-1], radius, edge, background)
    with np.errstate(invalid='ignore', divide='ignore'):
        mu = (w * x).sum((1, 2)) / w.sum() if demean else np.zeros(x.shape[0])
    return (x - mu[:, None, None]) * w, mu


def ring_sum(P2, n):
    """P2 [B][n][n] (a quantity per coefficient of the full plane) -> [B][Rr]: its sum over every ring."""
    idx = ring_index(n).reshape(-1)
    Rr = rings(n)
    return np.stack([np.bincount(idx, weights=p.reshape(-1), minlength=Rr) for p in P2])


def power(X, radius=None, edge=0.0, background=True, demean=True):
    """-> raw ring sums [B][Rr] of |fft2((x - mu) w)|^2, fp64."""
    y, _ = windowed(X, radius, edge, background, demean)
    return ring_sum(np.abs(np.fft.fft2(y)) ** 2, y.shape[-1])


def normalised(raw, n, radius=None, edge=0.0, background=True):
    """The raw sums as mean power per coefficient over sum w^2 (what tvae.spectrum.ring_power returns)."""
    w = window(n, radius, edge, background)
    return raw / (ring_counts(n) * (w * w).sum())


def windowed_f32(X, radius, edge, background, demean):
    """The kernel's input of stage 1: mu in fp64, (x - mu) rounded to fp32 once, times w in fp32."""
    x = np.asarray(X, dtype=np.float32)
    w = window(x.shape[-1], radius, edge, background)
    if demean:
        with np.errstate(invalid='ignore', divide='ignore'):
            mu = (w * x.astype(np.float64)).sum((1, 2)) / w.sum()
        x = (x.astype(np.float64) - mu[:, None, None]).astype(np.float32)
    return x * w.astype(np.float32)


def full_from_half(Ph, n):
    """[B][n][R] real, even under (ky, kx) -> (-ky, -kx) -> [B][n][n]."""
    return ctf_ref.full_plane(Ph, n)


def power_f32(X, radius=None, edge=0.0, background=True, demean=True):
    """Stages 1 and 2 in float32 numpy, |F|^2 in fp64 from the fp32 spectrum, the ring sums in fp64 -> [B][Rr]."""
    y = windowed_f32(X, radius, edge, background, demean)
    n = y.shape[-1]
    R = n // 2 + 1
    C, S = ctf_ref.twiddle_tables(n, np.float32)
    Gr, Gi = y @ C[:, :R], -(y @ S[:, :R])
    Fr, Fi = C @ Gr + S @ Gi, C @ Gi - S @ Gr
    p = Fr.astype(np.float64) ** 2 + Fi.astype(np.float64) ** 2
    return ring_sum(full_from_half(p, n), n)


def power_bound(X, radius=None, edge=0.0, background=True, demean=True):
    """The a-priori absolute bound [B][Rr] of test_spectrum_gpu.py's docstring on |kernel - power(...)|."""
    y, _ = windowed(X, radius, edge, background, demean)
    B, n = y.shape[0], y.shape[-1]
    R = n // 2 + 1
    g1, g2 = (n + 2) * EPS, (2 * n + 2) * EPS
    G = np.fft.fft(y, axis=-1)[..., :R]
    F = np.fft.fft(G, axis=-2)
    rows = np.sqrt((y ** 2).sum(2))                                        # |y_i|_2  [B][n]
    e_in = 3 * EPS * np.abs(y).sum((1, 2))                                 # [B]
    e1 = g1 * math.sqrt(n) * rows.sum(1)                                   # [B]: sum_i |E1(i, kx)|
    e1col = g1 * math.sqrt(n) * np.sqrt((y ** 2).sum((1, 2)))              # [B]: |E1(., kx)|_2
    gcol = np.sqrt((np.abs(G) ** 2).sum(1))                                # [B][R]
    e2 = math.sqrt(2) * g2 * math.sqrt(n) * (gcol + e1col[:, None])        # [B][R]
    e = (e_in + e1)[:, None, None] + e2[:, None, :]                        # [B][n][R] (the same for every ky)
    d = 2 * np.abs(F) * e + e * e
    ref = ring_sum(np.abs(np.fft.fft2(y)) ** 2, n)
    return ring_sum(full_from_half(d, n), n) + (ring_counts(n) + 2) * 2.0 ** -52 * ref


def group_sums(P, order, seg, N=None):
    """-> (sums fp64 [K][Rr], counts [K]): rows added in ascending position, entries of `order` outside [0, N) skipped,
    seg cleaned as the header states."""
    P = np.asarray(P, dtype=np.float64)
    N = P.shape[0] if N is None else N
    clean = np.minimum(np.maximum.accumulate(np.maximum(np.asarray(seg, dtype=np.int64), 0)), N)
    K = len(seg) - 1
    sums, counts = np.zeros((K, P.shape[1])), np.zeros(K, dtype=np.int64)
    for k in range(K):
        m = np.asarray(order[clean[k]:clean[k + 1]], dtype=np.int64)
        m = m[(m >= 0) & (m < N)]
        counts[k] = m.size
        for i in m:
            sums[k] = sums[k] + P[i]
    return sums, counts


def profile_plane(prof, n, interp):
    """prof [..][Rr] (the fp32 values as doubles) -> H [..][n][R] on the half spectrum: 0 nearest, 1 linear, the fp64 value."""
    p = np.asarray(prof, dtype=np.float64)
    R = n // 2 + 1
    ks = ctf_ref.signed(n)
    s2 = ks[:, None] ** 2 + np.arange(R)[None, :] ** 2
    if interp == 0:
        return p[..., ring_index(n)[:, :R]]
    s = np.sqrt(s2.astype(np.float64))
    r0 = np.minimum(np.floor(s).astype(np.int64), p.shape[-1] - 2)
    return p[..., r0] + (p[..., r0 + 1] - p[..., r0]) * (s - r0)


def radial_filter(X, prof, group, n, interp):
    """X [B][n][n], prof [G][Rr], group [B] or None -> fp64 [B][n][n]; a group outside [0, G) gives zeros.  H is the fp32
    rounding of the interpolated value, as the kernel multiplies with it."""
    prof = np.asarray(prof, dtype=np.float32).astype(np.float64)
    B = np.asarray(X).shape[0]
    g = np.zeros(B, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    ok = (g >= 0) & (g < prof.shape[0])
    H = profile_plane(prof[np.where(ok, g, 0)], n, interp).astype(np.float32).astype(np.float64)
    return np.where(ok[:, None, None], ctf_ref.filter(X, H), 0.0), H
