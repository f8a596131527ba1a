"""Eigenimages of the aligned classes on the GPU: tvae_class_project and tvae_class_backproject behind their C ABI (every call
under guard bands with replay, outputs and workspace filled with a sentinel) against the fp64 restatement tests/eigen_ref.py,
tvae.eigen.class_eigenimages on the planted case against the fp64 decomposition, and the TVAE_CLASS_EIGEN switch of the
clustering command line with class_eigenimages.py.

Tolerances against fp64.  With b_q the sampling bound of image q (test_align_gpu.image_bounds), m the mask and d the fp64
residual m (A - mean), a computed residual is within
    B = m b_q + 3 2^-24 |d|                  (the sample; the mask's rounding, the subtraction and the product)
of d.  project: |coef[q][j] - ref| <= sum_p B |V| + gamma 2^-24 sum_p |d V|, gamma = C ceil(n n / 256) + 8 the longest chain of
additions an output passes through in the order the header states (eigen_ref.chain); norm2 is the same with V = d.
backproject: |W - ref| <= sum_q |c_q| B_q + (chunk + 2) 2^-24 sum_q |c_q d_q| per element (a chain of at most `chunk` fp32
additions, the fp64 sum over the chunks and its rounding).  End to end, with R the class's fp64 residual matrix
(eigen_ref.planted_reference): dS = 2 |R|_F |B|_F + |B|_F^2 + 2 gamma 2^-24 |R|_F^2, |lambda_j - ref| <= 2 dS / (m - 1) (Weyl;
the factor 2 covers the second-order remainder), 1 - |cos(v_j, ref)| <= (2 dS / ((m - 1) gap_j))^2 (Davis-Kahan), the
coordinates up to sign within the project bound.  test_eigen_cpu.py checks on the reference alone that these are tight.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref
import eigen_ref as ER
import guardband
import test_align_gpu as TA
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 2.0 ** -24
SENT_F, SENT_I = -12345.5, -77777
N_IMG, K_CLS = TA.N_IMG, TA.K_CLS
MASKS = ('none', 'soft', 'hard')


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


def mask_of(kind, n):
    """(radius, edge): none, the soft mask ((n - 1) / 2 - 2, edge 2) and a hard edge."""
    return {'none': (0.0, 0.0), 'soft': ((n - 1) / 2 - 2, 2.0), 'hard': ((n - 1) / 2 - 1, 0.0)}[kind]


# ---- the C ABI under guard bands ---------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype).contiguous()


def run_project(Y, theta, dx, order, seg, mean, V, t, radius, edge, N=None):
    """tvae_class_project with sentinel-filled outputs and workspace -> numpy (coef [N][J], norm2 [N])."""
    from tvae import _cluster_lib as CL
    _, C, n, _ = Y.shape
    N = Y.shape[0] if N is None else N
    K, J = len(seg) - 1, V.shape[1]
    wsf = CL.query('tvae_class_project_ws_floats', N, K, C, n, J)
    assert wsf > 0
    ws = CL.workspace(wsf, DEV).fill_(SENT_F)
    coef, norm2 = torch.full((N, J), SENT_F, device=DEV), torch.full((N,), SENT_F, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_class_project', _dev(Y), _dev(theta), _dev(dx), _dev(order, torch.int32), _dev(seg, torch.int32),
                _dev(mean), _dev(V), coef, norm2, ws, wsf, N, C, n, K, J, t, radius, edge)
    return coef.cpu().numpy(), norm2.cpu().numpy()


def run_backproject(Y, theta, dx, order, seg, mean, coef, t, radius, edge, N=None):
    """tvae_class_backproject with sentinel-filled outputs and workspace -> numpy (W [K][J][C][n][n], counts [K])."""
    from tvae import _cluster_lib as CL
    _, C, n, _ = Y.shape
    N = Y.shape[0] if N is None else N
    K, J = len(seg) - 1, coef.shape[1]
    wsf = CL.query('tvae_class_backproject_ws_floats', N, K, C, n, J)
    assert wsf > 0
    ws = CL.workspace(wsf, DEV).fill_(SENT_F)
    W = torch.full((K, J, C, n, n), SENT_F, device=DEV)
    counts = torch.full((K,), SENT_I, dtype=torch.int32, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_class_backproject', _dev(Y), _dev(theta), _dev(dx), _dev(order, torch.int32), _dev(seg, torch.int32),
                _dev(mean), _dev(coef), W, counts, ws, wsf, N, C, n, K, J, t, radius, edge)
    return W.cpu().numpy(), counts.cpu().numpy()


# ---- references and bounds ---------------------------------------------------------------------------------------------------
def reference(aligned, bounds, mean, V, coef, order, seg, mk, n, C, chunk):
    """fp64 results and per-element bounds of both entry points for one set of inputs (V [K][J].., coef [N][J])."""
    N, K, J = aligned.shape[0], len(seg) - 1, V.shape[1]
    g = ER.chain(n, C)
    rc, rn = ER.project(aligned, mean, V, order, seg, mk)
    rW, rcnt = ER.backproject(aligned, mean, coef, order, seg, mk)
    bc, bn, bW = np.zeros((N, J)), np.zeros(N), np.zeros(rW.shape)
    mP = np.broadcast_to(mk[None], (C, n, n)).reshape(-1)
    for k in range(K):
        q, ids = ER.members(order, seg, k, N)
        if not q.size:
            continue
        D = np.abs(ER.residuals(aligned, mean, mk, ids, k).reshape(q.size, -1))
        B = bounds[ids][:, None] * mP[None, :] + 3 * EPS * D
        aV = np.abs(np.asarray(V[k], dtype=np.float64).reshape(J, -1))
        bc[q] = B @ aV.T + g * EPS * (D @ aV.T)
        bn[q] = (B * D).sum(1) + g * EPS * (D * D).sum(1)
        ac = np.abs(np.asarray(coef, dtype=np.float64)[q])
        bW[k] = (ac.T @ B + (chunk + 2) * EPS * (ac.T @ D)).reshape(bW[k].shape)
    return dict(coef=rc, norm2=rn, W=rW, counts=rcnt, b_coef=bc, b_norm2=bn, b_W=bW)


@functools.lru_cache(maxsize=None)
def inputs(n, C, J):
    """The stack, labels and poses of TA.case with the class averages of the fp64 reference rounded to fp32, a random block V
    and random coefficients."""
    c = TA.case(n, C)
    rng = np.random.default_rng(7000 * n + 10 * C + J)
    d = dict(c=c, mean=c['ref_avg'].astype(np.float32), V=rng.standard_normal((K_CLS, J, C, n, n)).astype(np.float32),
             coef=rng.standard_normal((N_IMG, J)).astype(np.float32))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(n, C, J, kind):
    """Reference (computed once, never modified) and guarded GPU results of one geometry, J and mask."""
    from tvae import _cluster_lib as CL
    i = inputs(n, C, J)
    c = i['c']
    radius, edge = mask_of(kind, n)
    chunk = CL.query('tvae_class_eigen_chunk', N_IMG, K_CLS, C, n, J)
    mk = ER.mask(n, radius, edge)
    ref = reference(c['ref'], c['bounds'], i['mean'], i['V'], i['coef'], c['order'], c['seg'], mk, n, C, chunk)
    got_c, got_n = run_project(c['Y'], c['theta'], c['dx'], c['order'], c['seg'], i['mean'], i['V'], c['t'], radius, edge)
    got_W, got_cnt = run_backproject(c['Y'], c['theta'], c['dx'], c['order'], c['seg'], i['mean'], i['coef'], c['t'], radius,
                                     edge)
    d = dict(ref, i=i, c=c, chunk=chunk, mask=mk, radius=radius, edge=edge, got_coef=got_c, got_norm2=got_n, got_W=got_W,
             got_counts=got_cnt)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def check_project(e, tag):
    err_c, err_n = np.abs(e['got_coef'] - e['coef']), np.abs(e['got_norm2'] - e['norm2'])
    live_c, live_n = e['b_coef'] > 0, e['b_norm2'] > 0
    print(f'project {tag}: worst error / bound coef {(err_c[live_c] / e["b_coef"][live_c]).max():.3f}, '
          f'norm2 {(err_n[live_n] / e["b_norm2"][live_n]).max():.3f}')
    assert not (e['got_coef'] == SENT_F).any() and not (e['got_norm2'] == SENT_F).any()
    assert (err_c <= e['b_coef']).all(), np.argwhere(err_c > e['b_coef'])[:10]
    assert (err_n <= e['b_norm2']).all(), np.flatnonzero(err_n > e['b_norm2'])[:10]


def check_backproject(e, tag):
    err = np.abs(e['got_W'] - e['W'])
    live = e['b_W'] > 0
    print(f'backproject {tag}: worst error / bound {(err[live] / e["b_W"][live]).max():.3f}')
    assert not (e['got_W'] == SENT_F).any()
    assert (err <= e['b_W']).all(), np.argwhere(err > e['b_W'])[:10]
    assert e['got_counts'].tolist() == e['counts'].tolist()


# ---- against fp64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('n,C', TA.GEOMETRIES)
def test_project_against_fp64(n, C, kind):
    e = case(n, C, 3, kind)
    assert e['c']['counts'].tolist() == [300, 1, 0, 60, 39] and 300 > 2 * e['chunk']     # the large class spans three chunks
    check_project(e, f'n={n} C={C} {kind}')
    assert np.abs(e['coef']).max() > 0 and (e['mask'] < 1).any() == (e['radius'] > 0)


@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('n,C', TA.GEOMETRIES)
def test_backproject_against_fp64(n, C, kind):
    e = case(n, C, 3, kind)
    check_backproject(e, f'n={n} C={C} {kind}')
    assert e['got_counts'].tolist() == [300, 1, 0, 60, 39]
    assert not e['got_W'][2].any()                                       # the empty class: zeros
    # the class of one: coef times its residual
    c, i = e['c'], e['i']
    q = int(c['seg'][1])
    d1 = ER.residuals(c['ref'], i['mean'], e['mask'], np.array([c['order'][q]]), 1)[0]
    want = i['coef'][q].astype(np.float64)[:, None, None, None] * d1[None]
    assert (np.abs(e['got_W'][1] - want) <= e['b_W'][1]).all()


@pytest.mark.parametrize('J', [1, 16])
@pytest.mark.parametrize('n,C', [(16, 1), (33, 3)])
def test_one_and_sixteen_components(n, C, J):
    e = case(n, C, J, 'soft')
    check_project(e, f'n={n} C={C} J={J}')
    check_backproject(e, f'n={n} C={C} J={J}')


# ---- hostile inputs ----------------------------------------------------------------------------------------------------------
def test_hostile_poses_give_minus_mask_times_mean():
    n, C, J, t = 16, 3, 3, 1.0
    i = inputs(n, C, J)
    c = TA.case(n, 1)                                                    # poses at t = 1
    rng = np.random.default_rng(77)
    Y = rng.standard_normal((N_IMG, C, n, n)).astype(np.float32)
    theta, dx = c['theta'].copy(), c['dx'].copy()
    hostile = np.array([12, 13, 20, 21, 22, 23, 24, 25, 399])
    theta[20] = np.nan
    dx[21], dx[22], dx[23] = (1e30, 0.0), (0.0, np.inf), (np.nan, 0.1)
    dx[24], dx[25], dx[399] = (-np.inf, np.inf), (-1e30, 1e30), (np.nan, np.nan)
    theta[399] = np.inf
    order, seg = c['order'], c['seg']
    A = align_ref.align_stack(Y, theta, dx, t)
    assert not A[hostile].any()
    bounds = TA.image_bounds(Y, dx, t, hostile)
    assert not bounds[hostile].any()
    radius, edge = mask_of('soft', n)
    mk = ER.mask(n, radius, edge)
    avg, _ = align_ref.class_averages(A, order, seg)
    mean = avg.astype(np.float32)
    from tvae import _cluster_lib as CL
    e = reference(A, bounds, mean, i['V'], i['coef'], order, seg, mk, n, C,
                  CL.query('tvae_class_eigen_chunk', N_IMG, K_CLS, C, n, J))
    e['got_coef'], e['got_norm2'] = run_project(Y, theta, dx, order, seg, mean, i['V'], t, radius, edge)
    e['got_W'], e['got_counts'] = run_backproject(Y, theta, dx, order, seg, mean, i['coef'], t, radius, edge)
    assert np.isfinite(e['got_coef']).all() and np.isfinite(e['got_W']).all()
    check_project(e, 'hostile poses')
    check_backproject(e, 'hostile poses')
    # their rows are those of d = -m * mean: the norm is the masked mean's, within the bound that has no sampling term
    pos = np.flatnonzero(np.isin(order, hostile))
    lab = np.searchsorted(seg, pos, side='right') - 1
    want = np.array([((mk[None] * mean[k].astype(np.float64)) ** 2).sum() for k in lab])
    assert (np.abs(e['got_norm2'][pos] - want) <= e['b_norm2'][pos]).all() and (e['b_norm2'][pos] <= 1e-5 * want).all()


def test_hostile_order_entries_give_zero_rows_and_are_not_counted():
    n, C, J = 16, 1, 3
    e0 = case(n, C, J, 'soft')
    c, i = e0['c'], e0['i']
    order = c['order'].copy()
    bad = [0, 5, 127, 128, 150, 299, 300, 301, 399]                      # in the large class, the class of one and the others
    order[bad] = [-1, N_IMG, -1, N_IMG, -(1 << 31), (1 << 31) - 1, -1, N_IMG + 1, N_IMG]
    e = reference(c['ref'], c['bounds'], i['mean'], i['V'], i['coef'], order, c['seg'], e0['mask'], n, C, e0['chunk'])
    e['got_coef'], e['got_norm2'] = run_project(c['Y'], c['theta'], c['dx'], order, c['seg'], i['mean'], i['V'], c['t'],
                                                e0['radius'], e0['edge'])
    e['got_W'], e['got_counts'] = run_backproject(c['Y'], c['theta'], c['dx'], order, c['seg'], i['mean'], i['coef'], c['t'],
                                                  e0['radius'], e0['edge'])
    assert not e['got_coef'][bad].any() and not e['got_norm2'][bad].any()
    assert e['got_counts'].tolist() == [294, 0, 0, 59, 38]
    check_project(e, 'hostile order')
    check_backproject(e, 'hostile order')
    assert not e['got_W'][1].any() and not e['got_W'][2].any()          # its only member skipped: an empty class
    keep = np.setdiff1d(np.arange(N_IMG), bad)
    assert np.array_equal(e['got_coef'][keep], e0['got_coef'][keep])     # the other rows do not notice


def test_hostile_seg_is_clamped_on_the_device():
    n, C, J = 16, 1, 3
    e0 = case(n, C, J, 'soft')
    c, i = e0['c'], e0['i']
    seg = np.array([-7, 120, 100, -5, 390, N_IMG + 1000])
    clean = np.array([0, 120, 120, 120, 390, N_IMG])
    args = (c['Y'], c['theta'], c['dx'], c['order'])
    tail = (c['t'], e0['radius'], e0['edge'])
    pc, pn = run_project(*args, seg, i['mean'], i['V'], *tail)
    qc, qn = run_project(*args, clean, i['mean'], i['V'], *tail)
    assert np.array_equal(pc, qc) and np.array_equal(pn, qn)
    W, cnt = run_backproject(*args, seg, i['mean'], i['coef'], *tail)
    W2, cnt2 = run_backproject(*args, clean, i['mean'], i['coef'], *tail)
    assert np.array_equal(W, W2) and cnt.tolist() == cnt2.tolist() == [120, 0, 0, 270, 10]
    e = reference(c['ref'], c['bounds'], i['mean'], i['V'], i['coef'], c['order'], clean, e0['mask'], n, C, e0['chunk'])
    e.update(got_coef=pc, got_norm2=pn, got_W=W, got_counts=cnt)
    check_project(e, 'hostile seg')
    check_backproject(e, 'hostile seg')
    # positions outside the cleaned [seg[0], seg[K]): exact zero rows
    short = np.array([10, 120, 120, 120, 200, 380])
    sc, sn = run_project(*args, short, i['mean'], i['V'], *tail)
    out = np.r_[0:10, 380:N_IMG]
    assert not sc[out].any() and not sn[out].any() and sc[10:380].any(axis=1).all()


def test_unsupported_arguments_are_rejected_and_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    N, C, n, K, J = 4, 1, 8, 2, 3
    Y = torch.zeros(N, C, n, n, device=DEV)
    th, dx = torch.zeros(N, device=DEV), torch.zeros(N, 2, device=DEV)
    order = torch.arange(N, dtype=torch.int32, device=DEV)
    seg = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    mean = torch.zeros(K, C, n, n, device=DEV)
    big = torch.full((K * 17 * C * n * n,), SENT_F, device=DEV)          # V, W and anything that overlaps them live here
    V = big[:K * J * C * n * n].view(K, J, C, n, n)
    coef, norm2 = torch.full((N, 17), SENT_F, device=DEV), torch.full((N,), SENT_F, device=DEV)
    W = torch.full((K, 17, C, n, n), SENT_F, device=DEV)
    counts = torch.full((K,), SENT_I, dtype=torch.int32, device=DEV)
    wsp, wsb = (CL.query(q, N, K, C, n, 16) for q in ('tvae_class_project_ws_floats', 'tvae_class_backproject_ws_floats'))
    ws = CL.workspace(max(wsp, wsb) + 2, DEV).fill_(SENT_F)
    assert ws.data_ptr() % 8 == 0 and ws[1:].data_ptr() % 8 == 4
    ok = dict(coef=coef, W=W, ws=ws, wsf=ws.numel(), n=n, J=J, radius=2.0, edge=1.0)
    variants = [dict(J=0), dict(J=17), dict(n=1), dict(radius=float('nan')), dict(edge=float('inf')), dict(edge=-1.0),
                dict(wsf=CL.query('tvae_class_project_ws_floats', N, K, C, n, J) - 1),                # a short workspace
                dict(ws=ws[1:], wsf=ws.numel() - 1),                                                  # a misaligned one
                dict(coef=big[8:8 + N * J].view(N, J), W=big[16:16 + K * J * C * n * n].view(K, J, C, n, n))]   # overlapping V
    for v in variants:
        a = dict(ok, **v)
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():                               # a rejected call must leave every tensor as it was
                CL.call('tvae_class_project', Y, th, dx, order, seg, mean, V, a['coef'], norm2, a['ws'], a['wsf'], N, C,
                        a['n'], K, a['J'], 1.0, a['radius'], a['edge'])
        if 'wsf' in v and 'ws' not in v:
            a['wsf'] = CL.query('tvae_class_backproject_ws_floats', N, K, C, n, J) - 1
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():
                # (W overlapping V: V is the block the host loop hands to the next projection; here it stands for any input, Y)
                CL.call('tvae_class_backproject', big[:N * C * n * n].view(N, C, n, n) if 'W' in v else Y, th, dx, order, seg,
                        mean, coef, a['W'], counts, a['ws'], a['wsf'], N, C, a['n'], K, a['J'], 1.0, a['radius'], a['edge'])
    for t in (big, coef, norm2, W, ws):
        assert (t == SENT_F).all()
    assert (counts == SENT_I).all()


# ---- reproducibility and independence ----------------------------------------------------------------------------------------
def test_python_api_is_bitwise_the_c_abi_and_reproducible():
    from tvae import eigen
    e = case(33, 3, 3, 'soft')
    c, i = e['c'], e['i']
    Y, th, dx = _dev(c['Y']), _dev(c['theta']).view(-1, 1), _dev(c['dx'])
    order, seg = _dev(c['order'], torch.int32), _dev(c['seg'], torch.int32)
    with guardband.GuardedCalls(replay=True):
        coef, norm2 = eigen.project(Y, th, dx, order, seg, _dev(i['mean']), _dev(i['V']), c['t'], e['radius'], e['edge'])
        W, cnt = eigen.backproject(Y, th, dx, order, seg, _dev(i['mean']), _dev(i['coef']), c['t'], e['radius'], e['edge'])
        coef2, norm22 = eigen.project(Y, th, dx, order, seg, _dev(i['mean']), _dev(i['V']), c['t'], e['radius'], e['edge'])
        W2, _ = eigen.backproject(Y, th, dx, order, seg, _dev(i['mean']), _dev(i['coef']), c['t'], e['radius'], e['edge'])
    assert np.array_equal(coef.cpu().numpy(), e['got_coef']) and np.array_equal(norm2.cpu().numpy(), e['got_norm2'])
    assert np.array_equal(W.cpu().numpy(), e['got_W']) and cnt.tolist() == e['got_counts'].tolist()
    assert torch.equal(coef, coef2) and torch.equal(norm2, norm22) and torch.equal(W, W2)
    assert cnt.dtype == torch.int32 and W.shape == (K_CLS, 3, 3, 33, 33) and coef.shape == (N_IMG, 3)
    # norm2 may be NULL: the coefficients do not notice
    from tvae import _cluster_lib as CL
    wsf = CL.query('tvae_class_project_ws_floats', N_IMG, K_CLS, 3, 33, 3)
    ws, alone = CL.workspace(wsf, DEV).fill_(SENT_F), torch.full((N_IMG, 3), SENT_F, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_class_project', Y, th.reshape(-1), dx, order, seg, _dev(i['mean']), _dev(i['V']), alone, None, ws, wsf,
                N_IMG, 3, 33, K_CLS, 3, c['t'], e['radius'], e['edge'])
    assert torch.equal(alone, coef)


def test_a_sub_stack_reproduces_its_rows_and_a_class_alone_its_block():
    e = case(16, 3, 3, 'soft')
    c, i = e['c'], e['i']
    order, seg = c['order'], c['seg']
    tail = (c['t'], e['radius'], e['edge'])
    # the members of classes 3 and 4 as a stack of their own: other N, other K, other positions, the same rows
    ids = order[seg[3]:seg[5]]
    sub_order = np.arange(ids.size)
    sub_seg = np.array([0, seg[4] - seg[3], seg[5] - seg[3]])
    pc, pn = run_project(c['Y'][ids], c['theta'][ids], c['dx'][ids], sub_order, sub_seg, i['mean'][3:5], i['V'][3:5], *tail)
    assert np.array_equal(pc, e['got_coef'][seg[3]:seg[5]]) and np.array_equal(pn, e['got_norm2'][seg[3]:seg[5]])
    # shifted by one position: the groups of four fall elsewhere, the rows stay
    one = np.r_[order[seg[3]], order[seg[3]:seg[5]]]
    pc1, _ = run_project(c['Y'], c['theta'], c['dx'], np.r_[one, np.zeros(N_IMG - one.size, int)],
                         np.array([0, 1, 1 + sub_seg[1], 1 + sub_seg[2]]), i['mean'][[3, 3, 4]], i['V'][[3, 3, 4]], *tail)
    assert np.array_equal(pc1[1:one.size], e['got_coef'][seg[3]:seg[5]])
    # class 0 alone (K = 1, its 300 members first): W[0] bit for bit; and class 3 alone at another position in `order`
    for k in (0, 3):
        m = seg[k + 1] - seg[k]
        alone = np.r_[order[seg[k]:seg[k + 1]], np.full(N_IMG - m, -1)]
        coef = np.zeros_like(i['coef'])
        coef[:m] = i['coef'][seg[k]:seg[k + 1]]
        W, cnt = run_backproject(c['Y'], c['theta'], c['dx'], alone, np.array([0, m]), i['mean'][k:k + 1], coef, *tail)
        assert np.array_equal(W[0], e['got_W'][k]) and cnt.tolist() == [m]


# ---- end to end --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(n, C):
    return ER.planted_reference(n, C, TA.image_bounds)


@pytest.mark.parametrize('n,C', [(33, 1), (16, 3)])
def test_eigenimages_of_the_planted_case(n, C):
    from tvae import eigen
    p = planted(n, C)
    m, J = p['m'], ER.PLANTED_J
    Y, th, dx = _dev(p['Y']), _dev(p['theta']), _dev(p['dx'])
    with guardband.GuardedCalls(replay=True):
        res = eigen.class_eigenimages(Y, th, dx, p['labels'].copy(), 1, components=J, oversample=4,
                                      power_iterations=ER.PLANTED_PASSES - 1, t_scale=p['t'], mean=_dev(p['mean']),
                                      mask_radius=p['radius'], mask_edge=p['edge'], seed=3)
    lam = res['eigenvalues'].cpu().numpy()[0]
    vec = res['eigenimages'].cpu().numpy()[0].reshape(J, -1).astype(np.float64)
    y = res['coordinates'].cpu().numpy().astype(np.float64)
    assert res['eigenvalues'].dtype == torch.float64 and res['counts'].tolist() == [m] and np.all(np.diff(lam) <= 0)
    assert np.allclose((vec * vec).sum(1), 1.0, atol=1e-6)
    g = ER.chain(n, C)
    absR = np.abs(p['R'])
    for j in range(3):
        cos = abs(vec[j] @ p['vec'][j]) / np.linalg.norm(vec[j])
        lam_err, sin2 = abs(lam[j] - p['lam'][j]), p['sine'][j] ** 2
        s = np.sign(vec[j] @ p['vec'][j])
        av = np.abs(p['vec'][j])
        b_y = p['B'] @ av + g * EPS * (absR @ av)
        y_err = np.abs(s * y[:, j] - p['coords'][:, j])
        print(f'planted n={n} C={C} component {j}: lambda error / tolerance {lam_err / p["lam_tol"]:.3e}, (1 - |cos|) / bound '
              f'{(1 - cos) / sin2:.3e}, worst coordinate error / bound {(y_err / b_y).max():.3f}')
        assert lam_err <= p['lam_tol']
        assert 1 - cos <= sin2
        assert (y_err <= b_y).all()
        top = np.argmax(np.abs(vec[j]))
        assert vec[j][top] > 0                                           # the sign convention
    tv = float(res['total_variance'][0])
    assert abs(tv - (p['R'] ** 2).sum() / (m - 1)) <= p['lam_tol']
    r = res['residual'].cpu().numpy()
    assert (r >= 0).all() and np.isfinite(r).all()


def test_rank_deficiency_gives_exact_zeros_and_no_nan():
    from tvae import eigen
    p = planted(16, 3)
    Y, th, dx = _dev(p['Y'][:6]), _dev(p['theta'][:6]), _dev(p['dx'][:6])
    labels = np.array([0, 0, 0, 1, 5, 2])                                # three members, one, none; image 4 in no class
    with guardband.GuardedCalls(replay=True):
        res = eigen.class_eigenimages(Y, th, dx, labels, 4, components=4, t_scale=p['t'], mask_radius=p['radius'],
                                      mask_edge=p['edge'])
    lam, E = res['eigenvalues'].cpu().numpy(), res['eigenimages'].cpu().numpy()
    assert np.isfinite(lam).all() and np.isfinite(E).all()
    assert (lam[0, :2] > 0).all() and not lam[0, 2:].any() and not E[0, 2:].any() and E[0, :2].any(axis=(1, 2, 3)).all()
    assert not lam[1:].any() and not E[1:].any()                         # fewer than two members: zeros
    y, r = res['coordinates'].cpu().numpy(), res['residual'].cpu().numpy()
    assert np.isnan(y[4]).all() and np.isnan(r[4]) and np.isfinite(np.delete(y, 4, 0)).all()
    assert not y[:3, 2:].any() and not y[[3, 5]].any() and res['counts'].tolist() == [3, 1, 1, 0]
    assert float(res['total_variance'][0]) > 0 and not res['total_variance'][1:].any()


# ---- the command lines -------------------------------------------------------------------------------------------------------
def test_clustering_particles_writes_the_eigen_files_and_class_eigenimages_py_reproduces_them(tmp_path):
    """clustering_particles.py on tests/golden/stack_ref.mrcs (5 images cropped to 6 x 6, MLP encoder, t = 0.1): with
    TVAE_CLASS_EIGEN=1 it adds the eigenimage files, unset the directory is what it was."""
    import src.models as M
    torch.manual_seed(2)
    enc = M.InferenceNetwork_UnimodalTranslation_UnimodalRotation(36, 2 + 3, 16, num_layers=2)
    torch.save(enc, tmp_path / 'inference.sav')
    stack = os.path.join(GOLDEN, 'stack_ref.mrcs')
    listing = {}
    for mode in ('off', 'on'):
        cmd = [sys.executable, os.path.join(PKG, 'clustering_particles.py'), '--test-path', stack, '--crop', '6',
               '--t-inf', 'unimodal', '--r-inf', 'unimodal', '--n-clusters', '2', '--path-to-encoder',
               str(tmp_path / 'inference.sav'), '--out-dir', str(tmp_path / mode)]
        env = dict(os.environ)
        for k in ('TVAE_CLASS_EIGEN', 'TVAE_CLASS_AVERAGES', 'TVAE_CLASS_FRC', 'TVAE_FIGURES'):
            env.pop(k, None)
        if mode == 'on':
            env['TVAE_CLASS_EIGEN'] = '1'
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert ('eigenimages' in r.stderr) == (mode == 'on')
        listing[mode] = sorted(os.listdir(tmp_path / mode))
    today = ['clusters.npy', 'latents.npy', 'results.txt', 'rotations.npy', 'translations.npy']
    assert listing['off'] == today
    files = ['class_eigen.txt', 'class_eigenimages.mrcs', 'class_eigenimages.npy', 'class_eigenvalues.npy',
             'eigen_coordinates.npy', 'eigen_residual.npy']
    extra = sorted(set(listing['on']) - set(today))
    assert extra in (files, sorted(files + ['class_eigenimages.jpg']))
    on = tmp_path / 'on'
    clusters = np.load(on / 'clusters.npy')
    E, lam = np.load(on / 'class_eigenimages.npy'), np.load(on / 'class_eigenvalues.npy')
    assert E.shape == (2, 4, 1, 6, 6) and E.dtype == np.float32 and lam.shape == (2, 4) and lam.dtype == np.float64
    assert np.isfinite(E).all() and np.isfinite(lam).all() and (np.diff(lam, axis=1) <= 0).all()
    for k in range(2):
        rank = min(max(int((clusters == k).sum()) - 1, 0), 4)            # m members about their own mean: rank m - 1
        assert (lam[k, :rank] > 0).all() and not lam[k, rank:].any() and not E[k, rank:].any()
    assert np.load(on / 'eigen_coordinates.npy').shape == (5, 4) and np.load(on / 'eigen_residual.npy').shape == (5,)
    assert len(open(on / 'class_eigen.txt').read().strip().split('\n')) == 4
    cmd = [sys.executable, os.path.join(PKG, 'class_eigenimages.py'), '--stack', stack, '--crop', '6', '--t-inf', 'unimodal',
           '--rotations', str(on / 'rotations.npy'), '--translations', str(on / 'translations.npy'),
           '--clusters', str(on / 'clusters.npy'), '--n-clusters', '2', '--out-dir', str(tmp_path / 'again')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    for f in files:
        assert open(tmp_path / 'again' / f, 'rb').read() == open(on / f, 'rb').read(), f
