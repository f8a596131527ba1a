"""t-SNE on the GPU: tvae_knn, tvae_tsne_repulsion, tvae_tsne_step and tvae_tsne_kl behind their C ABI (every entry point
under guard bands with replay, sentinel-filled padding and workspaces), fp64 NumPy references written here, tvae.tsne.tsne
against sklearn's Barnes-Hut TSNE, and the TVAE_FIGURES switch of the clustering command line.

u = 2^-24 throughout.

kNN, floats: the direct form sum_f (x_f - c_f)^2 carries d + 2 roundings relative to the distance itself; tol = 4 (d + 2) u,
twice the rigorous bound, as the Ward test does.

Repulsion: with A_i = sum_j q_ij^2 |y_i - y_j| (per component, fp64), |rep - rep64| <= (N + 16) u A_i holds for ANY order
of an fp32 sum of N terms whose own relative errors stay below 16 u; Z (all terms positive) within (N + 16) u relative.

Step: g = 4 (alpha attr - rep / Z).  The attraction is an fp32 sum over the row's entries, 2K roundings relative to
B_i = sum_e p_e q_e |y_i - y_col(e)|; rep and Z come from the repulsion kernel with the bounds above, |rep64| <= A_i, and
the closing operations (1 / Z rounded to fp32, one product each, one difference) add less than 4 u of each half:
    tol_g = 4 u (alpha (2K + 4) B_i + (2 (N + 16) + 4) A_i / Z).
"""
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import guardband
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
U = 2.0 ** -24
SENT_F, SENT_I = -12345.5, -77


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


def blobs(N, d, seed=0, centres=6, scale=6.0):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((centres, d)) * scale
    lab = np.arange(N) % centres
    return (C[lab] + rng.standard_normal((N, d))).astype(np.float32), lab


def _layout(X, ld=None, skew=0):
    """X [N][d] -> contiguous Xt [d][ld] on the device whose first element sits `skew` floats into its allocation; the
    padding holds a sentinel."""
    N, d = X.shape
    ld = (N + 3) // 4 * 4 if ld is None else ld
    store = torch.full((d * ld + skew,), SENT_F, device=DEV)
    Xt = store[skew:].view(d, ld)
    Xt[:, :N] = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV)
    return Xt, ld


def _odd(N):
    return N + 1 if (N + 1) % 4 else N + 3


def _d64(X):
    X = X.astype(np.float64)
    if X.shape[0] * X.shape[0] * X.shape[1] < 3e7:
        D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(2)
    else:
        D = np.stack([((X - x) ** 2).sum(1) for x in X])
    np.fill_diagonal(D, np.inf)
    return D


# ---- tvae_knn -------------------------------------------------------------------------------------------------------------
def _run_knn(X, K, ld=None, skew=0):
    from tvae import _cluster_lib as CL
    N, d = X.shape
    Xt, ld = _layout(X, ld, skew)
    idx = torch.full((N, K), SENT_I, dtype=torch.int32, device=DEV)
    d2 = torch.full((N, K), SENT_F, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_knn', Xt, ld, idx, d2, N, d, K)
    return Xt, idx.cpu().numpy(), d2.cpu().numpy()


def _knn_both_layouts(X, K):
    N = X.shape[0]
    Xa, ia, da = _run_knn(X, K)
    Xb, ib, db = _run_knn(X, K, ld=_odd(N), skew=1)
    assert Xa.shape[1] % 4 == 0 and Xa.data_ptr() % 16 == 0
    assert Xb.is_contiguous() and Xb.shape[1] % 4 != 0 and Xb.data_ptr() % 16 != 0
    # the scalar instance does the same arithmetic in the same order
    assert np.array_equal(ia, ib) and np.array_equal(da.view(np.int32), db.view(np.int32))
    return ia, da


KNN_EXACT = [(300, 4, 91, False), (92, 2, 91, False), (65, 1, 7, False), (1000, 16, 91, False), (4099, 4, 91, False),
             (300, 4, 91, True)]


@pytest.mark.parametrize('N,d,K,dup', KNN_EXACT)
def test_knn_exact_on_integer_points(N, d, K, dup):
    """Integer coordinates in [-8, 8]: every fp32 distance is exact and ties are plentiful, so idx and d2 have to equal the
    brute-force result sorted by (distance, index).  dup: every point occurs twice (a duplicate is a neighbour at 0)."""
    rng = np.random.default_rng(1000 * d + N + dup)
    if dup:
        half = rng.integers(-8, 9, (N // 2, d))
        X = np.concatenate([half, half]).astype(np.float32)
    else:
        X = rng.integers(-8, 9, (N, d)).astype(np.float32)
    X64 = X.astype(np.float64)
    sq = (X64 ** 2).sum(1)
    D = sq[:, None] + sq[None, :] - 2 * X64 @ X64.T                 # exact: small integers
    np.fill_diagonal(D, np.inf)
    want_idx = np.argsort(D, axis=1, kind='stable')[:, :K]
    want_d2 = np.take_along_axis(D, want_idx, 1)
    idx, d2 = _knn_both_layouts(X, K)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(d2.astype(np.float64), want_d2)
    if dup:
        h = N // 2
        assert (d2[:, 0] == 0).all() and (idx[:h, 0] <= np.arange(h) + h).all()


@pytest.mark.parametrize('N,d,K', [(257, 2, 91), (1000, 100, 91), (40, 256, 39)])
def test_knn_on_float_points(N, d, K):
    rng = np.random.default_rng(100 * d + N)
    X = rng.standard_normal((N, d)).astype(np.float32)
    D = _d64(X)
    kth = np.sort(D, axis=1)[:, K - 1]
    tol = 4 * (d + 2) * U
    idx, d2 = _knn_both_layouts(X, K)
    rows = np.arange(N)[:, None]
    assert ((idx >= 0) & (idx < N) & (idx != rows)).all()
    assert all(len(set(r.tolist())) == K for r in idx)
    got = D[rows, idx]
    worst = float((got.max(1) / kth).max() - 1)
    derr = float((np.abs(d2 - got) / got).max())
    print(f'knn {(N, d, K)}: worst returned d64 / K-th - 1 = {worst:.3e}, d2 error {derr:.3e}, bound {tol:.3e}')
    assert (got <= (kth * (1 + tol))[:, None]).all()
    member = np.zeros((N, N), bool)
    member[rows, idx] = True
    assert member[D < (kth * (1 - tol))[:, None]].all()
    assert (np.abs(d2 - got) <= tol * got).all()
    assert (np.diff(d2, axis=1) >= 0).all()


def test_knn_rejected_calls_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    Xt, ld = _layout(np.zeros((8, 3), np.float32))
    idx = torch.full((8, 7), SENT_I, dtype=torch.int32, device=DEV)
    d2 = torch.full((8, 7), SENT_F, device=DEV)
    g = guardband.GuardedCalls(replay=True)
    with g:
        for N, d, K, ldx in [(8, 3, 8, ld), (8, 3, 0, ld), (8, 257, 7, ld), (8, 0, 7, ld), (1, 3, 1, ld), (8, 3, 7, 7),
                             (300, 3, 257, 300)]:
            with pytest.raises(TvaeHipError):
                CL.call('tvae_knn', Xt, ldx, idx, d2, N, d, K)
    assert g.calls == 7 and not g.violations
    assert (idx == SENT_I).all() and (d2 == SENT_F).all()


# ---- tvae_tsne_repulsion --------------------------------------------------------------------------------------------------
def _rep64(Y):
    """fp64 all-pairs sums of the fp32 embedding Y [N][2]: (rep [N][2], A [N][2], Z)."""
    Y = Y.astype(np.float64)
    N = Y.shape[0]
    rep, A, Z = np.zeros((N, 2)), np.zeros((N, 2)), 0.0
    for r0 in range(0, N, 1024):
        dy = Y[r0:r0 + 1024, None, :] - Y[None, :, :]
        q = 1.0 / (1.0 + (dy ** 2).sum(2))
        q[np.arange(dy.shape[0]), r0 + np.arange(dy.shape[0])] = 0.0
        rep[r0:r0 + 1024] = (q[:, :, None] ** 2 * dy).sum(1)
        A[r0:r0 + 1024] = (q[:, :, None] ** 2 * np.abs(dy)).sum(1)
        Z += q.sum()
    return rep, A, Z


def _run_repulsion(Y, ld=None, skew=0):
    from tvae import _cluster_lib as CL
    N = Y.shape[0]
    Yt, ld = _layout(Y, ld, skew)
    rep = torch.full((2, ld), SENT_F, device=DEV)
    Z = torch.full((1,), SENT_F, dtype=torch.float64, device=DEV)
    wsf = CL.query('tvae_tsne_repulsion_ws_floats', N)
    assert wsf > 0
    ws = torch.full(((wsf + 1) // 2 * 2,), SENT_F, device=DEV)         # fp32 sentinels; the allocation is 8-byte aligned
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_tsne_repulsion', Yt, ld, rep, Z, ws, ws.numel(), N)
    assert (rep[:, N:] == SENT_F).all()
    return Yt, rep, Z


def _embedding(N, scale, seed, twins=False):
    Y = (np.random.default_rng(seed).standard_normal((N, 2)) * scale).astype(np.float32)
    if twins:
        Y[N - 3] = Y[5]
    return Y


@pytest.mark.parametrize('N,scale,twins', [(257, 1e-4, False), (1000, 1.0, False), (1000, 30.0, False), (4099, 10.0, False),
                                           (600, 3.0, True)])
def test_repulsion_against_fp64(N, scale, twins):
    Y = _embedding(N, scale, N + int(scale), twins)
    rep64, A, Z64 = _rep64(Y)
    bound = (N + 16) * U
    outs = []
    for name, ld, skew in (('aligned', None, 0), ('scalar', _odd(N), 1)):
        Yt, rep, Z = _run_repulsion(Y, ld, skew)
        got = rep[:, :N].t().cpu().numpy().astype(np.float64)
        z = float(Z)
        err = float((np.abs(got - rep64) / A).max())
        print(f'repulsion N={N} scale={scale} {name}: |rep - rep64| / A <= {err / U:.2f} u, |Z / Z64 - 1| = '
              f'{abs(z / Z64 - 1) / U:.2f} u, bound {(N + 16)} u')
        assert (np.abs(got - rep64) <= bound * A).all(), name
        assert abs(z - Z64) <= bound * Z64, name
        outs.append((got, z))
    # the scalar instance does the same arithmetic in the same order
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


def test_repulsion_with_several_column_tiles_per_workgroup():
    """Up to N = 16 384 every workgroup of the repulsion sees ONE column tile; above it a workgroup walks several: it
    stages again after the barrier, carries its accumulators and changes between the masked and the unmasked instance.
    N = 16 501 gives 65 row tiles x 17 ranges of 2 tiles (the last range has 1 tile, of 117 columns).  Sampled rows
    against fp64 with the bound of test_repulsion_against_fp64; Z over all pairs."""
    from tvae import _cluster_lib as CL
    N = 16501
    G = CL.query('tvae_tsne_groups', N)
    S = (CL.query('tvae_tsne_repulsion_ws_floats', N) - 2 * G) // (3 * N)
    assert S < (N + 511) // 512                                        # fewer ranges than tiles: several tiles per range
    Y = _embedding(N, 20.0, 17)
    rng = np.random.default_rng(3)
    rows = np.unique(np.concatenate([[0, 255, 256, 511, 512, 1023, 1024, 16383, 16384, N - 2, N - 1],
                                     rng.integers(0, N, 300)]))
    Y64 = Y.astype(np.float64)
    dy = Y64[rows, None, :] - Y64[None, :, :]
    q = 1.0 / (1.0 + (dy ** 2).sum(2))
    q[np.arange(rows.size), rows] = 0.0
    rep64 = (q[:, :, None] ** 2 * dy).sum(1)
    A = (q[:, :, None] ** 2 * np.abs(dy)).sum(1)
    x, y, Z64 = Y64[:, 0], Y64[:, 1], 0.0
    for r0 in range(0, N, 512):                                        # q is symmetric: the columns from r0 on suffice
        blk = 1.0 / (1.0 + (x[r0:r0 + 512, None] - x[None, r0:]) ** 2 + (y[r0:r0 + 512, None] - y[None, r0:]) ** 2)
        Z64 += blk[:, :512].sum() + 2.0 * blk[:, 512:].sum()
    Z64 -= N                                                           # the diagonal: q_ii = 1
    bound = (N + 16) * U
    outs = []
    for name, ld, skew in (('aligned', None, 0), ('scalar', _odd(N), 1)):
        Yt, rep, Z = _run_repulsion(Y, ld, skew)
        full = rep[:, :N].t().cpu().numpy()
        got = full[rows].astype(np.float64)
        z = float(Z)
        print(f'repulsion N={N} ({S} ranges) {name}: |rep - rep64| / A <= {float((np.abs(got - rep64) / A).max()) / U:.2f} u, '
              f'|Z / Z64 - 1| = {abs(z / Z64 - 1) / U:.2f} u, bound {N + 16} u')
        assert np.isfinite(full).all(), name
        assert (np.abs(got - rep64) <= bound * A).all(), name
        assert abs(z - Z64) <= bound * Z64, name
        outs.append((full, z))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


def test_repulsion_rejected_calls_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    N = 300
    Yt, ld = _layout(_embedding(N, 1.0, 0))
    rep = torch.full((2, ld), SENT_F, device=DEV)
    Z = torch.full((1,), SENT_F, dtype=torch.float64, device=DEV)
    wsf = CL.query('tvae_tsne_repulsion_ws_floats', N)
    ws = torch.full(((wsf + 1) // 2 * 2,), SENT_F, device=DEV)         # fp32 sentinels; the allocation is 8-byte aligned
    g = guardband.GuardedCalls(replay=True)
    with g:
        for n, ldy, wsn in [(1, ld, ws.numel()), (0, ld, ws.numel()), (N, N - 1, ws.numel()), (N, ld, wsf - 1)]:
            with pytest.raises(TvaeHipError, match='hipError_t 1'):
                CL.call('tvae_tsne_repulsion', Yt, ldy, rep, Z, ws, wsn, n)
    assert g.calls == 4 and not g.violations
    assert (rep == SENT_F).all() and (Z == SENT_F).all() and (ws == SENT_F).all()


# ---- tvae_tsne_step / tvae_tsne_kl ----------------------------------------------------------------------------------------
def _joint_p(N, d, seed):
    """CSR P of Gaussian blobs through the package's own host-side code (tests/test_tsne_cpu.py checks it against sklearn),
    on CPU tensors; returns (numpy rowptr, col, val, K)."""
    from tvae import tsne
    X, _ = blobs(N, d, seed)
    K = tsne.n_neighbors(N, 30.0)
    D = _d64(X)
    idx = np.argsort(D, axis=1, kind='stable')[:, :K]
    d2 = np.take_along_axis(D, idx, 1).astype(np.float32)
    P = tsne.joint_probabilities(torch.from_numpy(idx.astype(np.int32)),
                                 tsne.conditional_probabilities(torch.from_numpy(d2), 30.0))
    return P.rowptr.numpy(), P.col.numpy(), P.val.numpy(), K


@pytest.mark.parametrize('N', [257, 1000])
@pytest.mark.parametrize('alpha,momentum,scale', [(12.0, 0.5, 0.5), (1.0, 0.8, 8.0)])
def test_step_and_kl_against_fp64(N, alpha, momentum, scale):
    from tvae import _cluster_lib as CL
    lr = 200.0
    rowptr, col, val, K = _joint_p(N, 4, N)
    rng = np.random.default_rng(N + int(alpha))
    Y = _embedding(N, scale, N + 1)
    rep64, A, Z64 = _rep64(Y)
    Y64 = Y.astype(np.float64)
    # fp64 restatement
    row = np.repeat(np.arange(N), np.diff(rowptr))
    dy = Y64[row] - Y64[col]
    q = 1.0 / (1.0 + (dy ** 2).sum(1))
    pq = val.astype(np.float64) * q
    attr, B = np.zeros((N, 2)), np.zeros((N, 2))
    np.add.at(attr, row, pq[:, None] * dy)
    np.add.at(B, row, pq[:, None] * np.abs(dy))
    g64 = 4 * (alpha * attr - rep64 / Z64)
    p64 = val.astype(np.float64)
    eps = np.finfo(np.float64).eps
    kl64 = float((p64 * np.log(np.maximum(p64, eps) / np.maximum(q / Z64, eps))).sum())
    tol_g = 4 * U * (alpha * (2 * K + 4) * B + (2 * (N + 16) + 4) * A / Z64)
    # hand-set gains and update: both signs of update * grad, gains that the 0.8 factor takes below the floor
    gains = rng.uniform(0.5, 2.0, (N, 2)).astype(np.float32)
    gains[::7] = 0.011
    update = (np.sign(rng.standard_normal((N, 2))) * np.abs(g64) * rng.uniform(0.5, 50, (N, 2))).astype(np.float32)

    Yt, ld, = _layout(Y)
    _, rep, Z = _run_repulsion(Y)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    rp, cl, vl = dev(rowptr), dev(col), dev(val)

    def padded(a):
        t = torch.full((2, ld), SENT_F, device=DEV)
        t[:, :N] = dev(a.T)
        return t
    gains_d, update_d = padded(gains), padded(update)
    Yo = torch.full((2, ld), SENT_F, device=DEV)
    grad = torch.full((2, ld), SENT_F, device=DEV)
    G = CL.query('tvae_tsne_groups', N)
    gn2 = torch.full((G,), SENT_F, dtype=torch.float64, device=DEV)
    kl = torch.full((1,), SENT_F, dtype=torch.float64, device=DEV)
    klws = torch.full((G,), SENT_F, dtype=torch.float64, device=DEV)
    Y_before = Yt.clone()
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_tsne_kl', rp, cl, vl, val.size, Yt, ld, Z, kl, klws, G, N)
        CL.call('tvae_tsne_step', rp, cl, vl, val.size, Yt, rep, Z, gains_d, update_d, Yo, grad, gn2, ld, N, alpha,
                momentum, lr)
    assert torch.equal(Yt.view(torch.int32), Y_before.view(torch.int32))            # the input embedding, bit for bit
    for t in (gains_d, update_d, Yo, grad):
        assert (t[:, N:] == SENT_F).all()
    g = grad[:, :N].t().cpu().numpy()
    gerr = float((np.abs(g - g64) / tol_g).max())
    klerr = abs(float(kl) / kl64 - 1)
    print(f'step N={N} alpha={alpha}: |g - g64| <= {gerr:.3f} of the bound; KL {float(kl):.6f} (fp64 {kl64:.6f}, rel {klerr:.2e})')
    assert (np.abs(g - g64) <= tol_g).all()
    assert klerr <= 1e-5
    # the gain rule, wherever the sign of update * grad is decided beyond the bound
    inc64 = update.astype(np.float64) * g64 < 0
    decided = np.abs(update.astype(np.float64) * g64) > np.abs(update) * tol_g
    assert decided.mean() > 0.5 and inc64[decided].any() and (~inc64[decided]).any()
    want_gain = np.maximum(np.where(inc64, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01)).astype(np.float32)
    got_gain = gains_d[:, :N].t().cpu().numpy()
    assert np.array_equal(got_gain[decided], want_gain[decided])
    assert (got_gain[::7][decided[::7] & ~inc64[::7]] == np.float32(0.01)).all() and (decided[::7] & ~inc64[::7]).any()
    other = np.maximum(np.where(~inc64, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01)).astype(np.float32)
    assert ((got_gain == want_gain) | (got_gain == other)).all()
    # update = momentum * update - lr * gains * grad with the kernel's own gains and gradient (three roundings), then Y + update
    got_up = update_d[:, :N].t().cpu().numpy()
    want_up = momentum * update.astype(np.float64) - lr * got_gain.astype(np.float64) * g.astype(np.float64)
    mag = np.abs(momentum * update.astype(np.float64)) + np.abs(lr * got_gain.astype(np.float64) * g)
    assert (np.abs(got_up - want_up) <= 4 * U * mag).all()
    assert np.array_equal(Yo[:, :N].t().cpu().numpy(), Y + got_up)
    want_n2 = float((g.astype(np.float64) ** 2).sum())
    assert abs(float(gn2.sum()) - want_n2) <= 1e-12 * want_n2


def test_step_and_kl_rejected_calls_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    N = 64
    ld = 64
    rp = torch.arange(N + 1, dtype=torch.int32, device=DEV)
    cl = torch.zeros(N, dtype=torch.int32, device=DEV)
    vl = torch.full((N,), 1.0 / N, device=DEV)
    Yt = torch.randn(2, ld, device=DEV)
    outs = [torch.full((2, ld), SENT_F, device=DEV) for _ in range(4)]               # rep, gains, update, Yo
    Z = torch.ones(1, dtype=torch.float64, device=DEV)
    f64 = [torch.full((1,), SENT_F, dtype=torch.float64, device=DEV) for _ in range(3)]   # gn2, kl, klws
    g = guardband.GuardedCalls(replay=True)
    with g:
        for n, ldy, nnz in [(1, ld, N), (N, N - 1, N), (N, ld, 0)]:
            with pytest.raises(TvaeHipError, match='hipError_t 1'):
                CL.call('tvae_tsne_step', rp, cl, vl, nnz, Yt, outs[0], Z, outs[1], outs[2], outs[3], None, f64[0], ldy, n,
                        1.0, 0.5, 200.0)
            with pytest.raises(TvaeHipError, match='hipError_t 1'):
                CL.call('tvae_tsne_kl', rp, cl, vl, nnz, Yt, ldy, Z, f64[1], f64[2], 1, n)
        with pytest.raises(TvaeHipError, match='hipError_t 1'):                     # in place: refused
            CL.call('tvae_tsne_step', rp, cl, vl, N, Yt, outs[0], Z, outs[1], outs[2], Yt, None, f64[0], ld, N, 1.0, 0.5,
                    200.0)
        with pytest.raises(TvaeHipError, match='hipError_t 1'):                     # workspace too small
            CL.call('tvae_tsne_kl', rp, cl, vl, N, Yt, ld, Z, f64[1], f64[2], 0, N)
    assert g.calls == 8 and not g.violations
    assert all((t == SENT_F).all() for t in outs + f64)


# ---- tvae.tsne ------------------------------------------------------------------------------------------------------------
def test_gradient_and_pieces_of_the_python_api():
    from tvae import tsne
    N = 257
    X, _ = blobs(N, 4, N)
    Xd = torch.from_numpy(X).to(DEV)
    with guardband.GuardedCalls(replay=True):
        idx, d2 = tsne.knn(Xd, 91)
        P = tsne.joint_probabilities(idx, tsne.conditional_probabilities(d2, 30.0))
        Y = torch.from_numpy(_embedding(N, 2.0, 3)).to(DEV)
        grad, Z, kl = tsne.gradient(Y, P, 1.0)
    rowptr, col, val, _ = _joint_p(N, 4, N)
    assert np.array_equal(P.rowptr.cpu().numpy(), rowptr) and np.array_equal(P.col.cpu().numpy(), col)
    assert np.abs(P.val.cpu().numpy() - val).max() <= 1e-4 * val.max()
    rep64, A, Z64 = _rep64(Y.cpu().numpy())
    assert abs(Z / Z64 - 1) <= (N + 16) * U and tuple(grad.shape) == (N, 2) and kl > 0
    assert torch.equal(Y, torch.from_numpy(_embedding(N, 2.0, 3)).to(DEV))


def test_tsne_is_bitwise_reproducible_under_a_seed():
    from tvae import tsne
    X = torch.from_numpy(blobs(300, 4, 5)[0]).to(DEV)
    a = tsne.tsne(X, seed=11)
    b = tsne.tsne(X, seed=11)
    c = tsne.tsne(X, seed=12)
    assert a.n_iter == b.n_iter == 1000
    assert torch.equal(a.embedding.view(torch.int32), b.embedding.view(torch.int32)) and a.kl_divergence == b.kl_divergence
    assert not torch.equal(a.embedding, c.embedding)
    assert torch.isfinite(a.embedding).all() and tuple(a.embedding.shape) == (300, 2)


def test_tsne_refuses_what_it_cannot_do():
    from tvae import _lib, tsne
    from tvae._lib import TvaeHipError
    launches = []

    def hook(name, sig, args, do_call):
        launches.append(name)
        return do_call(args)

    old = _lib.set_call_hook(hook)
    try:
        with pytest.raises(TvaeHipError, match='perplexity'):
            tsne.tsne(torch.randn(30, 4, device=DEV))
        with pytest.raises(TvaeHipError):
            tsne.tsne(torch.randn(100, 257, device=DEV))
        with pytest.raises(TvaeHipError, match='init'):
            tsne.tsne(torch.randn(100, 4, device=DEV), init=torch.zeros(99, 2))
        X = torch.randn(100, 4, device=DEV)
        X[3, 1] = float('nan')
        with pytest.raises(TvaeHipError, match='NaN or Inf'):
            tsne.tsne(X)
        assert launches == []
    finally:
        _lib.set_call_hook(old)


def _kl64(rowptr, col, val, Y):
    Y = Y.astype(np.float64)
    N = Y.shape[0]
    Z = 0.0
    for r0 in range(0, N, 1024):
        q = 1.0 / (1.0 + ((Y[r0:r0 + 1024, None, :] - Y[None, :, :]) ** 2).sum(2))
        Z += q.sum() - q.shape[0]
    row = np.repeat(np.arange(N), np.diff(rowptr))
    q = 1.0 / (1.0 + ((Y[row] - Y[col]) ** 2).sum(1)) / Z
    p = val.astype(np.float64)
    eps = np.finfo(np.float64).eps
    return float((p * np.log(np.maximum(p, eps) / np.maximum(q, eps))).sum())


@pytest.mark.parametrize('N,d', [(600, 4), (1000, 8)])
def test_tsne_end_to_end_against_sklearn(N, d):
    """Gaussian blobs, the same explicit init for both; both embeddings are judged by ONE fp64 KL function over the same
    sparse P, by sklearn's trustworthiness and by the label purity of the 10 nearest embedded neighbours."""
    manifold = pytest.importorskip('sklearn.manifold')
    from tvae import tsne
    X, lab = blobs(N, d, N)
    Y0 = (1e-4 * np.random.default_rng(7).standard_normal((N, 2))).astype(np.float32)
    res = tsne.tsne(torch.from_numpy(X).to(DEV), init=torch.from_numpy(Y0))
    Yg = res.embedding.cpu().numpy()
    Ys = manifold.TSNE(2, learning_rate=200.0, init=Y0.copy(), perplexity=30.0).fit_transform(X)
    rowptr, col, val, _ = _joint_p(N, d, N)
    kg, ks = _kl64(rowptr, col, val, Yg), _kl64(rowptr, col, val, Ys)
    tg = manifold.trustworthiness(X, Yg, n_neighbors=10)
    ts = manifold.trustworthiness(X, Ys, n_neighbors=10)
    nn = np.argsort(_d64(Yg), axis=1)[:, :10]
    purity = float((lab[nn] == lab[:, None]).mean())
    print(f'tsne {(N, d)}: KL gpu {kg:.5f} sklearn {ks:.5f} ratio {kg / ks:.4f} (reported {res.kl_divergence:.5f}); '
          f'trustworthiness gpu {tg:.5f} sklearn {ts:.5f}; purity {purity:.4f}; {res.n_iter} iterations')
    assert np.isfinite(Yg).all() and abs(res.kl_divergence / kg - 1) <= 1e-4
    assert kg <= 1.10 * ks
    assert tg >= ts - 0.005
    assert purity >= 0.99


# ---- command line ---------------------------------------------------------------------------------------------------------
def test_clustering_mnist_cli_with_figures(tmp_path):
    """clustering_mnist.py on 48 synthetic images (perplexity 30 < N), once with TVAE_FIGURES=1 and once without: the switch
    adds tsne.npy and the figures and changes nothing else.  Only the two .jpg assertions need matplotlib."""
    have_mpl = importlib.util.find_spec('matplotlib') is not None
    import src.models as M
    rng = np.random.default_rng(0)
    n, zd, N = 32, 2, 48
    os.makedirs(tmp_path / 'data' / 'mnist_U')
    plain = np.zeros((N, 28, 28), np.uint8)
    labels = np.arange(N) % 3
    for i in range(N):                                     # three classes of bars / blocks
        c = labels[i]
        plain[i, 6 + 5 * c:12 + 5 * c, 4:24 - 6 * c] = 200 + rng.integers(0, 50)
    imgs = np.zeros((N, n, n), np.uint8)
    shifts = rng.integers(-2, 3, (N, 2))
    for i in range(N):
        imgs[i] = np.roll(np.pad(plain[i], 2), tuple(shifts[i]), (0, 1))
    np.save(tmp_path / 'data' / 'mnist_U' / 'images_test.npy', imgs)
    tr = np.concatenate([rng.uniform(-3, 3, (N, 1)), shifts[:, ::-1] * (2.0 / (n - 1))], 1)
    np.save(tmp_path / 'data' / 'mnist_U' / 'transforms_test.npy', tr)
    torch.save((torch.from_numpy(plain), torch.from_numpy(labels)), tmp_path / 'test.pt')
    torch.manual_seed(4)
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(
        n, 1, zd, kernels_num=8, kernels_size=n, padding=4, groupconv=8, rot_refinement=True, theta_prior=np.pi,
        normal_prior_over_r=False)
    os.makedirs(tmp_path / 'model')
    torch.save(enc, tmp_path / 'model' / 'inference.sav')
    err = {}
    for mode in ('figures', 'plain'):
        cmd = [sys.executable, os.path.join(PKG, 'clustering_mnist.py'), '--dataset', 'mnist-U', '--clustering', 'k-means',
               '--n-clusters', '3', '--n-init', '4', '--seed', '0', '--image-dim', str(n), '--minibatch-size', '10',
               '--path-to-encoder', 'model/inference.sav', '--path-to-mnist-test', 'test.pt', '--out-dir', mode]
        env = dict(os.environ)
        env.pop('TVAE_FIGURES', None)
        if mode == 'figures':
            env['TVAE_FIGURES'] = '1'
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        err[mode] = r.stderr
    assert 'figures of the reference are not built' in err['plain']
    assert 'not built' not in err['figures']
    assert '# saving tsne figure ... ' in err['figures']
    assert ('# saving confusion matrix ... ' in err['figures']) == have_mpl
    assert ('the figures are skipped' in err['figures']) == (not have_mpl)
    emb = np.load(tmp_path / 'figures' / 'tsne.npy')
    assert emb.shape == (N, 2) and np.isfinite(emb).all()
    for name in ('tsne.jpg', 'confusion_matrix.jpg'):
        if have_mpl:
            assert os.path.getsize(tmp_path / 'figures' / name) > 1000
        assert not os.path.exists(tmp_path / 'plain' / name)
    assert not os.path.exists(tmp_path / 'plain' / 'tsne.npy')
    for name in ('results.txt', 'latents.npy', 'clusters.npy'):
        assert open(tmp_path / 'figures' / name, 'rb').read() == open(tmp_path / 'plain' / name, 'rb').read(), name


def test_figures_step_without_matplotlib(tmp_path, monkeypatch, capsys):
    """The driver's figure step where matplotlib cannot be imported: tsne.npy is still written, stderr says that the figures
    were skipped, and no figure appears."""
    from tvae import cluster_driver
    monkeypatch.setitem(sys.modules, 'matplotlib', None)               # `import matplotlib` now raises ImportError
    N = 48
    X, lab = blobs(N, 2, 5, centres=3)
    z = torch.from_numpy(X).to(DEV)
    args = types.SimpleNamespace(seed=0, z_dim=2)
    cluster_driver._figures('mnist', args, str(tmp_path), z, None, None, lab.copy(), lab, (np.arange(3), np.arange(3)))
    err = capsys.readouterr().err
    assert 'the figures are skipped, tsne.npy is still written' in err and '# saving tsne figure ... ' in err
    assert '# saving confusion matrix' not in err
    emb = np.load(tmp_path / 'tsne.npy')
    assert emb.shape == (N, 2) and np.isfinite(emb).all()
    assert sorted(os.listdir(tmp_path)) == ['tsne.npy']
