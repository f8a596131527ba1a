"""fp64 restatement of the particle preprocessing from its definition (include/tvae_cluster.h): the Fourier downsample as
explicit DFT sums (no FFT, none of the reference's slicing), the sandwich product of given tables, the central crop and
the background-ring normalisation.  A plain helper module; imports nothing of the package."""
import numpy as np


def source_rows(M, m):
    """Source spectrum row of output spectrum row p: p for p < m // 2, M - m + p for every other p."""
    return [p if p < m // 2 else M - m + p for p in range(m)]


def column_weights(n):
    return [1.0 if kx == 0 or (n % 2 == 0 and kx == n // 2) else 2.0 for kx in range(n // 2 + 1)]


def downsample(x, shape):
    """x [..., M, N] -> [..., m, n], every sum written out."""
    x = np.asarray(x, dtype=np.float64)
    M, N = x.shape[-2:]
    m, n = shape
    a, b = np.arange(M), np.arange(N)
    Wy = np.stack([np.exp(-2j * np.pi * ((ky * a) % M) / M) for ky in source_rows(M, m)])            # [m][M]
    Wx = np.stack([np.exp(-2j * np.pi * ((kx * b) % N) / N) for kx in range(n // 2 + 1)])            # [n // 2 + 1][N]
    S = np.einsum('pa,...ab,kb->...pk', Wy, x, Wx)                                                   # F(src(p), kx)
    i, j = np.arange(m), np.arange(n)
    Ey = np.stack([np.exp(2j * np.pi * ((p * i) % m) / m) for p in range(m)])                        # [p][i]
    Ex = np.stack([w * np.exp(2j * np.pi * ((kx * j) % n) / n) for kx, w in enumerate(column_weights(n))])
    return np.einsum('pi,...pk,kj->...ij', Ey, S, Ex).real / (M * N)


def complex_tables(M, N, m, n):
    """(Ry [m][M], Kx [N][n]) as complex fp64 arrays, summed term by term."""
    i, a = np.arange(m)[:, None], np.arange(M)[None, :]
    Ry = sum(np.exp(2j * np.pi * (((p * i * M - s * a * m) % (m * M)) / (m * M))) for p, s in enumerate(source_rows(M, m)))
    b, j = np.arange(N)[:, None], np.arange(n)[None, :]
    Kx = sum(w * np.exp(2j * np.pi * (((kx * (j * N - b * n)) % (n * N)) / (n * N))) for kx, w in enumerate(column_weights(n)))
    return Ry, Kx


def sandwich(x, Ar, Ai, Br, Bi, scale):
    """scale (Ar x Br - Ai x Bi) in fp64; Ai = Bi = None skips the second term."""
    x = np.asarray(x, dtype=np.float64)
    out = np.asarray(Ar, dtype=np.float64) @ x @ np.asarray(Br, dtype=np.float64)
    if Ai is not None:
        out = out - np.asarray(Ai, dtype=np.float64) @ x @ np.asarray(Bi, dtype=np.float64)
    return scale * out


def sandwich_bound(x, Ar, Ai, Br, Bi, scale):
    """|Ar| |x| |Br| + |Ai| |x| |Bi|, times |scale|: what the a-priori error bound of the kernel is relative to."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    out = np.abs(np.asarray(Ar, dtype=np.float64)) @ x @ np.abs(np.asarray(Br, dtype=np.float64))
    if Ai is not None:
        out = out + np.abs(np.asarray(Ai, dtype=np.float64)) @ x @ np.abs(np.asarray(Bi, dtype=np.float64))
    return abs(scale) * out


def crop(stack, size):
    n, m = stack.shape[-2:]
    si, sj = (n - size) // 2, (m - size) // 2
    return stack[..., si:si + size, sj:sj + size]


def ring_mask(n, m, radius=None):
    """(n / 2 - i)^2 + (m / 2 - j)^2 >= radius^2; default radius min(n, m) / 2."""
    r = min(n, m) / 2 if radius is None else float(radius)
    i, j = np.arange(n)[:, None], np.arange(m)[None, :]
    return (n / 2 - i) ** 2 + (m / 2 - j) ** 2 >= r * r


def normalize(stack, radius=None):
    """stack [B][n][m] -> (normalised fp64 [B][n][m], stats fp64 [B][2] = (mean, population std) of the masked pixels)."""
    x = np.asarray(stack, dtype=np.float64)
    B, n, m = x.shape
    mask = ring_mask(n, m, radius)
    out, stats = np.empty_like(x), np.empty((B, 2))
    with np.errstate(all='ignore'):
        for b in range(B):
            v = x[b][mask]
            mu = v.sum() / v.size if v.size else np.nan
            sd = np.sqrt(((v - mu) ** 2).sum() / v.size) if v.size else np.nan
            out[b] = (x[b] - mu) / sd
            stats[b] = mu, sd
    return out, stats
