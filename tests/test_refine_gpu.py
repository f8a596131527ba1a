"""Pose refinement against the class averages on the GPU: tvae_pose_refine behind its C ABI (every call under guard bands with
replay, outputs and workspace filled with a sentinel) against the fp64 restatement tests/pose_ref.py, tvae.refine, and
refine_poses.py.

Tolerance of the tables against fp64 (poses: the fp32 values converted to double), built as image_bounds of
test_align_gpu.py is.  The position at which a template pixel reads the reference is about a dozen fp32 roundings away from
the exact one (the grid coordinate and its step, t dx, the difference, two products and their sum per axis, the two sincos
errors, the shift to pixels and its scale), each relative to a quantity of size at most
    Mg = 1 + 2 (X + t |dx_i|_inf),  X = 1 + 2 S / (n - 1) the half width of the extended grid in coordinate units,
that is (n - 1) / 2 times as much in pixels:
    delta_i = 16 * 2^-24 * Mg * (n - 1) / 2                                    (pixels per axis)
    b_i = 2 g_k delta_i + 4 * 2^-24 * max |ref_k|                               per template sample (k the image's class)
with g_k the largest difference between adjacent pixels of the zero-bordered reference.  Under a soft mask the distance from
the centre is off by at most sqrt(2) delta_i, the raised cosine has the slope pi / (2 edge) at most, and the mask and its
product are rounded once each:  b_i += max |ref_k| (pi / (2 edge) sqrt(2) delta_i + 2 * 2^-24).
Through the sums, with gamma = m 2^-24 / (1 - m 2^-24) for the m = C n^2 terms of a sum in whatever order:
    |d num| <= b_i sum |Y| + gamma sum |P| |Y|,   |d pp| <= 2 b_i sum |P| + m b_i^2 + gamma sum P^2,   |d yy| <= gamma sum Y^2.
Where the fp64 template of an image is zero throughout (out of frame, a hostile pose, a skipped image) the bound is 0: exact
zeros are required.  No constant was tuned against the kernel.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref
import guardband
import pose_ref
import test_align_gpu as TA
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 2.0 ** -24
SENT_F = -12345.5
SENT_I = -7777777
N_IMG, K_CLS = 24, 4
# (n, C, A, S, N): odd n; S and A at their limits; the LDS limit
GEOMETRIES = [(8, 1, 1, 1, N_IMG), (17, 2, 2, 3, N_IMG), (32, 3, 8, 2, N_IMG), (33, 1, 0, 8, N_IMG), (64, 1, 32, 0, N_IMG),
              (128, 1, 2, 3, 3)]
CASES = [g + (m,) for g in GEOMETRIES for m in (False, True)]
HOSTILE = (20, 21, 22, 23)


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype).contiguous()


def run_refine(Y, theta, dx, cls, refs, A, S, t, dtheta, radius=0.0, edge=0.0, tables=True):
    """tvae_pose_refine into sentinel-filled outputs and workspace -> dict of numpy arrays."""
    from tvae import _cluster_lib as CL
    N, C, n, _ = Y.shape
    K, NA, NS = refs.shape[0], 2 * A + 1, 2 * S + 1
    wsf = CL.query('tvae_pose_refine_ws_floats', N, C, n, A, S)
    assert wsf == N * (2 * NA * NS * NS + 1)
    ws = torch.full((wsf,), SENT_F, device=DEV)
    th_out, dx_out, score = (torch.full(s, SENT_F, device=DEV) for s in ((N,), (N, 2), (N, 2)))
    best = torch.full((N, 3), SENT_I, dtype=torch.int32, device=DEV)
    num = pp = yy = None
    if tables:
        num, pp, yy = (torch.full(s, SENT_F, device=DEV) for s in ((N, NA, NS, NS), (N, NA, NS, NS), (N,)))
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_refine', _dev(Y), _dev(theta), _dev(dx), _dev(cls, torch.int32), _dev(refs), th_out, dx_out, score,
                best, num, pp, yy, ws, wsf, N, C, n, K, A, S, t, dtheta, radius, edge)
    out = dict(theta=th_out, dx=dx_out, score=score, best=best, num=num, pp=pp, yy=yy)
    out = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    for k, v in out.items():
        assert not (v == (SENT_I if k == 'best' else SENT_F)).any(), k
    return out


def make_inputs(n, C, N, seed):
    """The poses of test_align_gpu.make_poses (special angles, whole-pixel shifts, half and fully out of frame, large shifts) with
    four hostile ones, labels in K = 4 classes with class 2 empty and two labels outside [0, K)."""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, C, n, n)).astype(np.float32)
    refs = rng.standard_normal((K_CLS, C, n, n)).astype(np.float32)
    theta, dx = TA.make_poses(rng, n, N=40)
    theta, dx = theta[:N].copy(), dx[:N].copy()
    cls = rng.choice([0, 1, 3], N)
    if N == N_IMG:
        theta[20] = np.nan
        dx[21], dx[22], dx[23] = (1e30, 0.0), (0.0, np.inf), (np.nan, 0.1)
        cls[5], cls[17] = -1, 7
        cls[:3] = [0, 1, 3]
    return Y, refs, theta, dx, cls


def table_bounds(c):
    n, C, S, t, ref = c['n'], c['C'], c['S'], c['t'], c['ref']
    K = c['refs'].shape[0]
    cls = c['cls']
    valid = (cls >= 0) & (cls < K)
    kk = np.where(valid, cls, 0)
    X = 1 + 2 * S / (n - 1)
    with np.errstate(invalid='ignore', over='ignore'):
        Mg = 1 + 2 * (X + np.float64(np.float32(t)) * np.abs(c['dx'].astype(np.float64)).max(1))
        delta = 16 * EPS * Mg * (n - 1) / 2
        rmax = np.abs(c['refs']).max(axis=(1, 2, 3))[kk]
        b = 2 * TA.adjacent_step(c['refs'])[kk] * delta + 4 * EPS * rmax
        if c['radius'] > 0:
            b = b + rmax * (np.pi / (2 * c['edge']) * np.sqrt(2) * delta + 2 * EPS)
    dead = ~np.abs(ref['T']).reshape(cls.size, -1).any(1)                # exact zeros are required there
    b = np.where(dead, 0.0, b)
    assert np.isfinite(b).all() and dead[~valid].all()
    m = C * n * n
    gamma = m * EPS / (1 - m * EPS)
    aT = np.abs(ref['T'])
    absnum, _, _ = pose_ref.tables(np.abs(c['Y']), aT, S)
    sumP, _, _ = pose_ref.tables(np.ones_like(c['Y']), aT, S)
    sumY = np.abs(c['Y'].astype(np.float64)).sum(axis=(1, 2, 3))
    b4 = b[:, None, None, None]
    return dict(num=b4 * sumY[:, None, None, None] + gamma * absnum, pp=2 * b4 * sumP + m * b4 * b4 + gamma * ref['pp'],
                yy=gamma * ref['yy'], dead=dead)


def score_bounds(ref, bnd):
    """|d score| from the bounds of the three sums (first order, the fp32 rounding of the score added); inf where a bound is not
    small against its sum."""
    num, pp = ref['num'], ref['pp']
    yy = ref['yy'][:, None, None, None]
    byy = bnd['yy'][:, None, None, None]
    with np.errstate(invalid='ignore', divide='ignore'):
        ok = (pp > 0) & (yy > 0) & (bnd['pp'] < 0.5 * pp)
        den = np.sqrt(np.where(ok, pp * yy, 1.0))
        s = np.abs(num) / den
        e = bnd['num'] / den + s * (bnd['pp'] / np.where(ok, pp, 1.0) + byy / np.where(ok, yy, 1.0)) + EPS * s
    zero = (pp == 0) | (yy == 0)
    return np.where(zero, 0.0, np.where(ok, 1.01 * e, np.inf))


@functools.lru_cache(maxsize=None)
def case(n, C, A, S, N, masked):
    """Inputs, the fp64 reference (computed once, never modified) and the guarded GPU results of one geometry.  Every second
    geometry runs at t = 0.1 with the translations scaled by 10, as the unimodal encoder reports them."""
    t = 1.0 if n in (8, 32, 64) else 0.1
    dtheta = 0.02 if A > 8 else 0.05
    radius, edge = (0.3 * n, max(2.0, 0.15 * n)) if masked else (0.0, 0.0)
    Y, refs, theta, dx, cls = make_inputs(n, C, N, 100 * n + C)
    dx = (dx / np.float32(t)).astype(np.float32)
    t64 = float(np.float32(t))
    ref = pose_ref.refine(Y, theta, dx, cls, refs, t64, A, dtheta, S, radius if masked else None, edge)
    got = run_refine(Y, theta, dx, cls, refs, A, S, t, dtheta, radius, edge)
    c = dict(n=n, C=C, A=A, S=S, N=N, t=t, dtheta=dtheta, radius=radius, edge=edge, Y=Y, refs=refs, theta=theta, dx=dx,
             cls=cls, ref=ref, got=got)
    c['bounds'] = table_bounds(c)
    for d in (c, ref, got, c['bounds']):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c


# ---- 1. the tables against fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C,A,S,N,masked', CASES)
def test_tables_against_fp64(n, C, A, S, N, masked):
    c = case(n, C, A, S, N, masked)
    ref, got, bnd = c['ref'], c['got'], c['bounds']
    for nm in ('num', 'pp', 'yy'):
        err = np.abs(got[nm] - ref[nm])
        live = bnd[nm] > 0
        worst = (err[live] / bnd[nm][live]).max() if live.any() else 0.0
        print(f'pose_refine n={n} C={C} A={A} S={S} t={c["t"]} mask={masked} {nm}: worst error {err.max():.3e}, worst error / bound '
              f'{worst:.3f}')
        assert (err <= bnd[nm]).all(), (nm, np.argwhere(err > bnd[nm])[:5])
    dead = bnd['dead']
    assert not got['num'][dead].any() and not got['pp'][dead].any()      # out of frame, hostile, skipped: exact zeros
    if N == N_IMG:
        assert dead[list(HOSTILE)].all() and dead[[5, 17]].all() and not dead[:5].any()
        assert not got['yy'][[5, 17]].any() and got['yy'][0] > 0


# ---- 2. the selection ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C,A,S,N,masked', CASES)
def test_selection_is_the_rule_on_the_gpu_scores(n, C, A, S, N, masked):
    c = case(n, C, A, S, N, masked)
    ref, got = c['ref'], c['got']
    K = c['refs'].shape[0]
    sc = pose_ref.scores(got['num'], got['pp'], got['yy'])               # fp64 from the GPU's fp32 sums, rounded once
    best, out = pose_ref.select(sc, c['cls'], K)
    th, dx = pose_ref.update_pose(c['theta'], c['dx'], best, n, c['t'], c['dtheta'])
    assert np.array_equal(got['best'], best)
    assert np.array_equal(got['score'].view(np.int32), out.view(np.int32))
    assert np.array_equal(got['theta'].view(np.int32), th.view(np.int32)) and np.array_equal(got['dx'].view(np.int32), dx.view(np.int32))
    assert (got['score'][:, 1] >= got['score'][:, 0]).all()
    keep = (got['best'] == 0).all(1)
    assert np.array_equal(got['theta'][keep].view(np.int32), c['theta'][keep].view(np.int32))
    assert np.array_equal(got['dx'][keep].view(np.int32), c['dx'][keep].view(np.int32))
    # the fp64 score at the GPU's choice is within the bounds of the fp64 maximum
    e = score_bounds(ref, c['bounds'])
    s64 = np.where(ref['pp'] == 0, 0.0, ref['num'] / np.sqrt(np.where(ref['pp'] == 0, 1.0, ref['pp'] * ref['yy'][:, None, None, None])))
    NS = 2 * S + 1
    flat = lambda a, i: a[i].reshape(-1)
    for i in np.flatnonzero((c['cls'] >= 0) & (c['cls'] < K)):
        g = ((got['best'][i, 0] + A) * NS + got['best'][i, 1] + S) * NS + got['best'][i, 2] + S
        r = int(np.argmax(flat(s64, i)))
        assert flat(s64, i)[g] >= flat(s64, i)[r] - flat(e, i)[g] - flat(e, i)[r], (i, g, r)


def test_hard_mask_edge_smoke():
    c = case(17, 2, 2, 3, N_IMG, False)
    got = run_refine(c['Y'], c['theta'], c['dx'], c['cls'], c['refs'], 2, 3, c['t'], c['dtheta'], 5.0, 0.0)
    assert np.isfinite(got['num']).all() and np.isfinite(got['pp']).all() and (got['pp'] <= c['got']['pp'] * (1 + 1e-5) + 1e-6).all()
    assert (got['score'][:, 1] >= got['score'][:, 0]).all()


# ---- 3. recovery -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [1.0, 0.1])
def test_planted_poses_are_recovered(t):
    p = pose_ref.planted(t=t)
    got = run_refine(p['Y'], p['theta'], p['dx'], p['cls'], p['refs'], p['A'], p['S'], t, p['dtheta'])
    assert np.array_equal(got['best'], p['want']), np.flatnonzero((got['best'] != p['want']).any(1))
    assert (got['score'][:, 1] > 1 - 1e-4).all()
    assert np.abs(got['dx'].astype(np.float64) - p['dx_true']).max() <= 4e-7 / t


# ---- 4. skipped images -------------------------------------------------------------------------------------------------------------
def test_skipped_images_and_the_empty_class():
    c = case(32, 3, 8, 2, N_IMG, False)
    got = c['got']
    skipped = [5, 17]
    assert np.array_equal(got['theta'][skipped].view(np.int32), c['theta'][skipped].view(np.int32))
    assert np.array_equal(got['dx'][skipped].view(np.int32), c['dx'][skipped].view(np.int32))
    assert not got['score'][skipped].any() and not got['best'][skipped].any()
    args = (c['A'], c['S'], c['t'], c['dtheta'])
    # every reference NaN: nothing of ref is read for a skipped image
    nan = run_refine(c['Y'], c['theta'], c['dx'], c['cls'], np.full_like(c['refs'], np.nan), *args)
    for k in ('theta', 'dx', 'score', 'best', 'num', 'pp', 'yy'):
        assert np.array_equal(nan[k][skipped].view(np.int32), got[k][skipped].view(np.int32)), k
    # the empty class's reference NaN: nothing changes for anybody, its neighbours 1 and 3 included
    refs = c['refs'].copy()
    refs[2] = np.nan
    assert (c['cls'] != 2).all() and (c['cls'] == 1).any() and (c['cls'] == 3).any()
    other = run_refine(c['Y'], c['theta'], c['dx'], c['cls'], refs, *args)
    for k in other:
        assert np.array_equal(other[k].view(np.int32), got[k].view(np.int32)), k


# ---- 5. independence and reproducibility -------------------------------------------------------------------------------------------
def test_independent_of_the_other_images_and_of_K_and_reproducible():
    from tvae import refine
    c = case(17, 2, 2, 3, N_IMG, True)
    got = c['got']
    args = (c['A'], c['S'], c['t'], c['dtheta'], c['radius'], c['edge'])
    again = run_refine(c['Y'], c['theta'], c['dx'], c['cls'], c['refs'], *args)
    for k in got:
        assert np.array_equal(again[k].view(np.int32), got[k].view(np.int32)), k
    sub = np.array([19, 3, 4, 9, 16, 0, 22])
    part = run_refine(c['Y'][sub], c['theta'][sub], c['dx'][sub], c['cls'][sub], c['refs'], *args)
    more = run_refine(c['Y'], c['theta'], c['dx'], np.where(c['cls'] == 7, 9, c['cls']),
                      np.concatenate([c['refs'], np.ones_like(c['refs'])]), *args, tables=False)
    for k in got:
        assert np.array_equal(part[k].view(np.int32), got[k][sub].view(np.int32)), k
        if k in more:
            assert np.array_equal(more[k].view(np.int32), got[k].view(np.int32)), k
    # the Python API is bitwise the C ABI
    with guardband.GuardedCalls(replay=True):
        api = refine.refine_poses(_dev(c['Y']), _dev(c['theta']).view(-1, 1), _dev(c['dx']), c['cls'].copy(), _dev(c['refs']),
                                  c['t'], c['A'], c['dtheta'], c['S'], c['radius'], c['edge'], tables=True)
    for v, k in zip(api, ('theta', 'dx', 'score', 'best', 'num', 'pp', 'yy')):
        assert np.array_equal(v.cpu().numpy().view(np.int32), got[k].view(np.int32)), k
    assert api[3].dtype == torch.int32 and api[0].shape == (N_IMG,) and len(refine.refine_poses(
        _dev(c['Y']), _dev(c['theta']), _dev(c['dx']), torch.from_numpy(c['cls'].copy()), _dev(c['refs']), c['t'], 1, None, 1)) == 4


# ---- 6. rejection ------------------------------------------------------------------------------------------------------------------
def test_unsupported_arguments_are_rejected_and_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    N, C, n, K, A, S = 4, 1, 8, 2, 1, 1
    Y, refs = torch.zeros(N, C, n, n, device=DEV), torch.zeros(K, C, n, n, device=DEV)
    th, dx = torch.zeros(N, device=DEV), torch.zeros(N, 2, device=DEV)
    cls = torch.zeros(N, dtype=torch.int32, device=DEV)
    wsf = CL.query('tvae_pose_refine_ws_floats', N, C, n, A, S)
    outs = [torch.full(s, SENT_F, device=DEV) for s in ((N,), (N, 2), (N, 2))]
    best = torch.full((N, 3), SENT_I, dtype=torch.int32, device=DEV)
    num, pp = (torch.full((N, 3, 3, 3), SENT_F, device=DEV) for _ in range(2))
    yy, ws = torch.full((N,), SENT_F, device=DEV), torch.full((wsf,), SENT_F, device=DEV)

    def attempt(N=N, C=C, n=n, K=K, A=A, S=S, t=1.0, dth=0.1, radius=0.0, edge=0.0, th_out=outs[0], num=num, pp=pp, wsf=wsf):
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():                               # a rejected call must leave every tensor as it was
                CL.call('tvae_pose_refine', Y, th, dx, cls, refs, th_out, outs[1], outs[2], best, num, pp, yy, ws, wsf, N, C, n,
                        K, A, S, t, dth, radius, edge)

    for kw in (dict(n=129), dict(A=33), dict(S=9), dict(C=17), dict(t=0.0), dict(dth=float('nan')), dict(pp=None),
               dict(th_out=th), dict(wsf=wsf - 1), dict(n=1), dict(N=0), dict(K=0), dict(K=65536), dict(A=-1), dict(S=-1),
               dict(t=float('inf')), dict(t=-1.0), dict(dth=float('inf')), dict(num=None), dict(edge=-1.0),
               dict(radius=float('nan')), dict(edge=float('inf'))):
        attempt(**kw)
    for t_ in outs + [num, pp, yy, ws]:
        assert (t_ == SENT_F).all()
    assert (best == SENT_I).all()
    for bad in [(N, C, 129, A, S), (N, C, n, 33, S), (N, C, n, A, 9), (N, 17, n, A, S)]:
        assert CL.query('tvae_pose_refine_ws_floats', *bad) == 0


# ---- 7. refine_rounds end to end -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blurred_start():
    """60 noise-free images of 3 planted references, the starting poses off by up to 10 degrees and 2 pixels."""
    p = pose_ref.planted(seed=21, N=60)
    rng = np.random.default_rng(22)
    n = p['n']
    theta0 = (p['theta_true'] + np.radians(rng.uniform(-10, 10, 60))).astype(np.float32)
    dx0 = (p['dx_true'] + rng.uniform(-2, 2, (60, 2)) * 2 / (n - 1)).astype(np.float32)
    return p, theta0, dx0


def test_refine_rounds_sharpens_the_averages():
    from tvae import align, refine
    p, theta0, dx0 = blurred_start()
    Y, th0, d0 = _dev(p['Y']), _dev(theta0), _dev(dx0)
    K = p['K']
    with guardband.GuardedCalls(replay=True):
        th, d, hist = refine.refine_rounds(Y, th0, d0, p['cls'], K, 1.0, rounds=3, angle_range=np.pi / 8, angle_steps=8, shift=2)
    sc = hist['scores']
    print('refine_rounds: mean centre / best score per round', sc.tolist(), 'steps', hist['steps'])
    assert hist['steps'] == [np.pi / 64, np.pi / 128, np.pi / 256]
    assert sc.shape == (3, 2) and (sc[:, 1] >= sc[:, 0]).all() and sc[0, 1] < sc[1, 1] < sc[2, 1] and sc[2, 1] > sc[0, 0]
    start = align.class_averages(Y, th0, d0, p['cls'], K, 1.0)[0].cpu().numpy().astype(np.float64)
    final = align.class_averages(Y, th, d, p['cls'], K, 1.0)[0].cpu().numpy().astype(np.float64)
    l2 = lambda a: np.sqrt(((a - p['refs']) ** 2).sum(axis=(1, 2, 3)))
    print('refine_rounds: L2 distance of the class averages from the planted references', l2(start).tolist(), '->', l2(final).tolist())
    assert (l2(final) < l2(start)).all()


def test_cross_halves_never_score_an_image_against_an_average_that_contains_it():
    """One round with cross_halves: an image of half 0 is scored against the half-1 average of its class, so altering OTHER
    images of half 0 leaves its result bit for bit; the images of half 1, whose reference those images are part of, do change."""
    from tvae import refine
    p, theta0, dx0 = blurred_start()
    K = p['K']
    which = pose_ref.cross_half_labels(p['cls'], K)
    half0 = np.flatnonzero(which >= K)
    half1 = np.flatnonzero((which >= 0) & (which < K))
    altered = half0[::3]
    Y2 = p['Y'].copy()
    Y2[altered] = np.random.default_rng(3).standard_normal(Y2[altered].shape).astype(np.float32)
    res = []
    for y in (p['Y'], Y2):
        with guardband.GuardedCalls(replay=True):
            th, d, _ = refine.refine_rounds(_dev(y), _dev(theta0), _dev(dx0), p['cls'], K, 1.0, rounds=1, cross_halves=True)
        res.append((th.cpu().numpy(), d.cpu().numpy()))
    same = np.setdiff1d(half0, altered)
    assert same.size and np.array_equal(res[0][0][same].view(np.int32), res[1][0][same].view(np.int32))
    assert np.array_equal(res[0][1][same].view(np.int32), res[1][1][same].view(np.int32))
    assert not (np.array_equal(res[0][0][half1], res[1][0][half1]) and np.array_equal(res[0][1][half1], res[1][1][half1]))


# ---- 8. the command line -------------------------------------------------------------------------------------------------------
def test_refine_poses_py_writes_its_files_and_class_averages_py_reproduces_the_averages(tmp_path):
    p = pose_ref.planted(seed=31, N=5, n=16, K=2)
    rng = np.random.default_rng(32)
    np.save(tmp_path / 'stack.npy', p['Y'][:, 0])
    np.save(tmp_path / 'rotations.npy', (p['theta_true'] + rng.uniform(-0.1, 0.1, 5)).astype(np.float32).reshape(5, 1))
    np.save(tmp_path / 'translations.npy', (p['dx_true'] + rng.uniform(-0.1, 0.1, (5, 2))).astype(np.float32))
    np.save(tmp_path / 'clusters.npy', p['cls'])
    files = ['--stack', str(tmp_path / 'stack.npy'), '--clusters', str(tmp_path / 'clusters.npy'), '--n-clusters', '2']
    cmd = [sys.executable, os.path.join(PKG, 'refine_poses.py'), *files, '--rotations', str(tmp_path / 'rotations.npy'),
           '--translations', str(tmp_path / 'translations.npy'), '--out-dir', str(tmp_path / 'out'), '--rounds', '2',
           '--angle-steps', '4', '--shift', '1']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / 'out'
    listing = sorted(os.listdir(out))
    assert listing in (['class_averages_refined.jpg', 'class_averages_refined.npy', 'refine_scores.npy', 'rotations_refined.npy',
                        'translations_refined.npy'],
                       ['class_averages_refined.npy', 'refine_scores.npy', 'rotations_refined.npy', 'translations_refined.npy'])
    lines = [ln for ln in r.stdout.splitlines() if not ln.startswith('#')]
    assert len(lines) == 2 and all(ln.count('->') == 2 for ln in lines)  # one line per class: both resolutions before -> after
    rot, tr = np.load(out / 'rotations_refined.npy'), np.load(out / 'translations_refined.npy')
    assert rot.shape == (5, 1) and rot.dtype == np.float32 and tr.shape == (5, 2) and np.load(out / 'refine_scores.npy').shape == (2, 2)
    avg = np.load(out / 'class_averages_refined.npy')
    assert avg.shape == (2, 1, 16, 16) and avg.dtype == np.float32
    cmd = [sys.executable, os.path.join(PKG, 'class_averages.py'), *files, '--rotations', str(out / 'rotations_refined.npy'),
           '--translations', str(out / 'translations_refined.npy'), '--out-dir', str(tmp_path / 'again')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.array_equal(np.load(tmp_path / 'again' / 'class_averages.npy'), avg)
