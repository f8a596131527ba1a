"""Sub-pixel pose polish on the GPU: tvae_pose_moments and tvae_pose_polish_step behind their C ABI (every call under guard bands
with replay, outputs filled with a sentinel) against the fp64 restatement tests/polish_ref.py, tvae.polish, and polish_poses.py.

Tolerance of the moments against fp64 (poses: the fp32 values converted to double), in the manner of table_bounds of
test_refine_gpu.py.  The position at which a pixel reads the reference is off by at most
    delta_i = 16 * 2^-24 * Mg * (n - 1) / 2   pixels per axis,   Mg = 1 + 2 (1 + t |dx_i|_inf)      (S = 0 there).
With, for the zero-bordered reference of the image's class k, g_k the largest first difference, x_k the largest mixed second
difference, j_k the largest second difference along one axis and r_k = max |ref_k|, and h = (n - 1) / 2:
    value      eB = 2 g_k delta_i + 4 * 2^-24 r_k                                        (b_i of test_refine_gpu.py)
    derivative eD = x_k delta_i + 4 * 2^-24 g_k       Bc and Br are continuous within a cell and move with the other axis'
                                                      weight by the mixed difference; |Bc|, |Br| <= g_k
               eD = j_k + x_k delta_i + 4 * 2^-24 g_k for a sample whose fp64 col or row lies within delta_i of an integer: the
                                                      fp32 kernel may legitimately sit in the neighbouring cell, and across a
                                                      cell edge the derivative along that axis jumps by a second difference
    mask       em = pi / (2 edge) sqrt(2) delta_i + 2 * 2^-24   (0 without a mask), as there
    P:   eB + r_k em         G0, G1:  eG = h (eD + 2 * 2^-24 g_k + g_k em)
    Dtheta = -u1 G0 + u0 G1 with |u| <= U = 2 (1 + t |dx_i|_inf), u off by delta_i / h:
         eT = 2 U eG + 2 delta_i g_k + 6 * 2^-24 U h g_k.
Through a sum of m = C n^2 products f g with gamma = m 2^-24 / (1 - m 2^-24), in whatever order:
    |d sum| <= sum (|f| eg + |g| ef + ef eg) + gamma sum (|f| + ef) (|g| + eg)            (as pp is bounded there; eY = 0).
Where the fp64 template and its derivatives are zero throughout (out of frame, a hostile pose, a skipped image) the bound of
the first 14 sums is 0: exact zeros are required.  No constant was tuned against the kernel.

The edge rule cannot hide a failure: over the images with generic poses (angles and shifts drawn from continuous
distributions) at most 1 % of the samples may be flagged -- the expected share is about 4 delta_i -- and that is asserted on
the fp64 reference alone before the kernel's numbers are looked at.  The lattice poses of make_poses (theta a multiple of pi / 2
with whole-pixel shifts: every sample sits on a cell corner) are exempt from the cap; for them only the sums without a
derivative (PP, PY, YY) carry a tight bound.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guardband
import polish_ref
import pose_ref
import test_refine_gpu as TR
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 2.0 ** -24
SENT_F = -12345.5
SENT_I = -7777777
F32 = np.float32
N_IMG = TR.N_IMG
# (n, C, N): odd n, the LDS limit
GEOMETRIES = [(8, 1, N_IMG), (17, 2, N_IMG), (32, 3, N_IMG), (33, 1, N_IMG), (64, 1, N_IMG), (128, 1, 3)]
CASES = [g + (m,) for g in GEOMETRIES for m in (False, True)]
HOSTILE = TR.HOSTILE
SKIPPED = (5, 17)
LATTICE = (0, 1, 2, 3, 6, 7)            # theta a multiple of pi / 2 with whole-pixel shifts (test_align_gpu.make_poses)
I = polish_ref.IDX
MAX_SHIFT, MAX_ANGLE, ITERATIONS = 1.0, 0.05, 8


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


def run_moments(Y, theta, dx, cls, refs, t, radius=0.0, edge=0.0):
    """tvae_pose_moments into a sentinel-filled output -> mom [N][15] (numpy fp32)."""
    from tvae import _cluster_lib as CL
    N, C, n, _ = Y.shape
    mom = torch.full((N, 15), SENT_F, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_moments', _dev(Y), _dev(theta), _dev(dx), _dev(cls, torch.int32), _dev(refs), mom, N, C, n,
                refs.shape[0], t, radius, edge)
    out = mom.cpu().numpy()
    assert not (out == SENT_F).any()
    return out


STATE = ('theta_try', 'dx_try', 'theta', 'dx', 'mom', 'score', 'lam', 'steps', 'ended')


def new_gpu_state(N):
    f = lambda *s: torch.full(s, SENT_F, device=DEV)
    i = lambda *s: torch.full(s, SENT_I, dtype=torch.int32, device=DEV)
    return dict(theta_try=f(N), dx_try=f(N, 2), theta=f(N), dx=f(N, 2), mom=f(N, 15), score=f(N, 2),
                lam=torch.full((N,), SENT_F, dtype=torch.float64, device=DEV), steps=i(N), ended=i(N))


def run_step(st, cls, theta0, dx0, mom_try, n, K, first, t, max_shift=MAX_SHIFT, max_angle=MAX_ANGLE):
    """tvae_pose_polish_step on the device state `st` (tensors, changed in place)."""
    from tvae import _cluster_lib as CL
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_polish_step', cls, theta0, dx0, mom_try, *(st[k] for k in STATE), cls.numel(), n, K, int(first), t,
                max_shift, max_angle)


def host_state(st):
    """The device state as a polish_ref state dict (the moments converted to double)."""
    h = {k: v.cpu().numpy().copy() for k, v in st.items()}
    h['mom'] = h['mom'].astype(np.float64)
    h['exact'] = [None] * h['theta'].size
    return h


def second_differences(refs):
    """Per reference: (g, x, j) = the largest first, mixed second and one-axis second difference of the zero-bordered planes
    (two zeros to every side, so that the steps into and out of the border count)."""
    P = np.pad(np.asarray(refs, dtype=np.float64), ((0, 0), (0, 0), (2, 2), (2, 2)))
    ax = (1, 2, 3)
    g = np.maximum(np.abs(np.diff(P, axis=2)).max(axis=ax), np.abs(np.diff(P, axis=3)).max(axis=ax))
    x = np.abs(np.diff(np.diff(P, axis=2), axis=3)).max(axis=ax)
    j = np.maximum(np.abs(np.diff(P, n=2, axis=2)).max(axis=ax), np.abs(np.diff(P, n=2, axis=3)).max(axis=ax))
    return g, x, j


def moment_bounds(c):
    """-> dict(mom [N][15] the bounds, dead [N], flagged [N][n][n])."""
    n, C, t, b = c['n'], c['C'], c['t'], c['basis']
    K = c['refs'].shape[0]
    cls = c['cls']
    valid = (cls >= 0) & (cls < K)
    kk = np.where(valid, cls, 0)
    h = (n - 1) / 2
    g, x, j = (v[kk][:, None, None] for v in second_differences(c['refs']))
    rmax = np.abs(c['refs']).max(axis=(1, 2, 3))[kk][:, None, None]
    with np.errstate(invalid='ignore', over='ignore'):
        shift = np.float64(F32(t)) * np.abs(c['dx'].astype(np.float64)).max(1)
        delta = (16 * EPS * (1 + 2 * (1 + shift)) * h)[:, None, None]
        U = (2 * (1 + shift))[:, None, None]
        col, row = b['pos']['col'], b['pos']['row']
        flagged = (np.abs(col - np.rint(col)) <= delta) | (np.abs(row - np.rint(row)) <= delta)
        flagged &= np.isfinite(col) & np.isfinite(row) & (np.abs(col) < 4 * n) & (np.abs(row) < 4 * n)
        em = (np.pi / (2 * c['edge']) * np.sqrt(2) * delta + 2 * EPS) if c['radius'] > 0 else 0 * delta
        eP = 2 * g * delta + 4 * EPS * rmax + rmax * em
        eD = x * delta + 4 * EPS * g + np.where(flagged, j, 0.0)
        eG = h * (eD + 2 * EPS * g + g * em)
        eT = 2 * U * eG + 2 * delta * g + 6 * EPS * U * h * g
    dead = ~(np.abs(b['P']).reshape(cls.size, -1).any(1) | np.abs(b['G0']).reshape(cls.size, -1).any(1) |
             np.abs(b['G1']).reshape(cls.size, -1).any(1))
    assert dead[~valid].all()
    m = C * n * n
    gamma = m * EPS / (1 - m * EPS)
    f = dict(P=np.abs(b['P']), D=np.abs(b['D']), G0=np.abs(b['G0']), G1=np.abs(b['G1']), Y=np.abs(c['Y'].astype(np.float64)))
    zero = np.zeros_like(eP)
    e = {k: np.where(dead[:, None, None], 0.0, v)[:, None] for k, v in dict(P=eP + zero, D=eT + zero, G0=eG + zero, G1=eG + zero,
                                                                           Y=zero).items()}
    assert all(np.isfinite(v).all() for v in e.values())
    pairs = (('P', 'P'), ('P', 'D'), ('P', 'G0'), ('P', 'G1'), ('D', 'D'), ('D', 'G0'), ('D', 'G1'), ('G0', 'G0'), ('G0', 'G1'),
             ('G1', 'G1'), ('P', 'Y'), ('D', 'Y'), ('G0', 'Y'), ('G1', 'Y'), ('Y', 'Y'))
    s = lambda a: a.sum(axis=(1, 2, 3))
    bound = np.stack([s(f[p] * e[q] + f[q] * e[p] + e[p] * e[q]) + gamma * s((f[p] + e[p]) * (f[q] + e[q])) for p, q in pairs], 1)
    bound[dead, :14] = 0.0
    bound[~valid] = 0.0
    return dict(mom=bound, dead=dead, flagged=flagged, valid=valid, eP=e['P'])


@functools.lru_cache(maxsize=None)
def case(n, C, N, masked):
    """Inputs (test_refine_gpu.make_inputs), the fp64 reference (computed once, never modified), its bounds and the guarded GPU
    moments of one geometry.  Every second geometry runs at t = 0.1 with the translations scaled by 10."""
    t = 1.0 if n in (8, 32, 64) else 0.1
    radius, edge = (0.3 * n, max(2.0, 0.15 * n)) if masked else (0.0, 0.0)
    Y, refs, theta, dx, cls = TR.make_inputs(n, C, N, 100 * n + C)
    dx = (dx / F32(t)).astype(F32)
    basis = polish_ref.basis(refs, cls, theta, dx, t, radius if masked else None, edge)
    ref = polish_ref.moments(Y, basis)
    c = dict(n=n, C=C, N=N, t=t, radius=radius, edge=edge, Y=Y, refs=refs, theta=theta, dx=dx, cls=cls, basis=basis, ref=ref)
    c['bounds'] = moment_bounds(c)
    # the cap on the edge rule, on the fp64 reference alone and before the kernel runs
    bnd = c['bounds']
    generic = [i for i in range(N) if i not in LATTICE and not bnd['dead'][i]]
    share = bnd['flagged'][generic].mean() if generic else 0.0          # (the three images of n = 128 are lattice poses)
    c['flag_share'] = share
    assert len(generic) >= (10 if N == N_IMG else 0) and share <= 0.01, (n, C, share)
    c['got'] = run_moments(Y, theta, dx, cls, refs, t, radius, edge)
    for d in (c, bnd):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c


# ---- 1. the moments against fp64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C,N,masked', CASES)
def test_moments_against_fp64(n, C, N, masked):
    c = case(n, C, N, masked)
    ref, got, bnd = c['ref'], c['got'], c['bounds']
    err = np.abs(got.astype(np.float64) - ref)
    live = bnd['mom'] > 0
    ratio = np.where(live, err / np.where(live, bnd['mom'], 1.0), 0.0)
    tight = [i for i in range(N) if i not in LATTICE and not bnd['dead'][i] and not bnd['flagged'][i].any()]
    rel = (bnd['mom'][tight] / np.maximum(np.abs(ref[tight]), 1e-300)) if tight else np.zeros((1, 15))
    print(f'pose_moments n={n} C={C} t={c["t"]} mask={masked}: flagged share {c["flag_share"]:.2e}, worst error / bound per moment '
          f'{np.round(ratio.max(0), 3).tolist()}; median bound / |moment| on unflagged images '
          f'{np.array2string(np.median(rel, 0), precision=1)}')
    assert (err <= bnd['mom']).all(), np.argwhere(err > bnd['mom'])[:8]
    dead = bnd['dead']
    assert not got[dead, :14].any()                                      # out of frame, hostile, skipped: exact zeros
    if N == N_IMG:
        assert dead[list(HOSTILE)].all() and dead[list(SKIPPED)].all() and not dead[:5].any()
        assert not got[list(SKIPPED)].any() and (got[list(HOSTILE), 14] > 0).all()
    # yy is tvae_pose_refine's bit for bit, and PP and PY are its centre candidate up to the order of addition
    tr = TR.run_refine(c['Y'], c['theta'], c['dx'], c['cls'], c['refs'], 0, 0, c['t'], 0.0, c['radius'], c['edge'])
    assert np.array_equal(tr['yy'].view(np.int32), got[:, 14].view(np.int32))
    m = C * n * n
    gamma = m * EPS / (1 - m * EPS)
    # (the same fp32 products in two orders: each sum is within gamma of the exact sum of those products' magnitudes)
    pp_r, num_r = tr['pp'][:, 0, 0, 0].astype(np.float64), tr['num'][:, 0, 0, 0].astype(np.float64)
    sumPY = ((np.abs(c['basis']['P']) + bnd['eP']) * np.abs(c['Y'].astype(np.float64))).sum(axis=(1, 2, 3))
    assert (np.abs(pp_r - got[:, 0]) <= 2 * gamma * np.maximum(pp_r, got[:, 0]) / (1 - gamma)).all()
    assert (np.abs(num_r - got[:, 10]) <= 2 * gamma * sumPY * (1 + 2 * EPS)).all()


def test_hard_mask_edge_smoke():
    c = case(17, 2, N_IMG, False)
    got = run_moments(c['Y'], c['theta'], c['dx'], c['cls'], c['refs'], c['t'], 5.0, 0.0)
    assert np.isfinite(got).all() and (got[:, 0] <= c['got'][:, 0] * (1 + 1e-5) + 1e-6).all()
    assert np.array_equal(got[:, 14].view(np.int32), c['got'][:, 14].view(np.int32))


# ---- 2. the step against its restatement -------------------------------------------------------------------------------------------
def _far_from_a_boundary(w):
    """Is the fp64 value w further than 2^-20 of an fp32 step from the two fp32 rounding boundaries around it?  Both sides do the
    same correctly rounded fp64 operations in the same order on the same inputs (c and s among them: the correctly rounded fp32
    cosine and sine), so the fp64 values should agree to the last bit; 2^-20 of an fp32 step is 2^9 fp64 steps of slack."""
    f = F32(w)
    up, dn = np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))
    d = min(abs(w - (float(f) + float(up)) / 2), abs(w - (float(f) + float(dn)) / 2))
    return d > 2.0 ** -20 * min(float(up) - float(f), float(f) - float(dn))


def _ulps(a, b):
    ia, ib = F32(a).view(np.int32).astype(np.int64), F32(b).view(np.int32).astype(np.int64)
    key = lambda i: np.where(i < 0, -(i & 0x7fffffff), i)
    return int(abs(key(ia) - key(ib)))


@pytest.mark.parametrize('n,C,N,masked', [(17, 2, N_IMG, True), (32, 3, N_IMG, False), (64, 1, N_IMG, False)])
def test_step_kernel_is_its_restatement_on_the_kernels_own_moments(n, C, N, masked):
    """Planted images with off-grid starts in the first 16 slots, the hostile and skipped poses of the moments cases behind them.
    Every step call is compared with polish_ref.step from the SAME device state and the same fp32 moments: decisions, lambda,
    steps, scores and the ended flags are identical; a trial is identical in bits wherever its fp64 value is far from an fp32
    rounding boundary (2^-20 of an fp32 step, see _far_from_a_boundary) and within one fp32 step otherwise."""
    c = case(n, C, N, masked)
    t, K = c['t'], c['refs'].shape[0]
    rng = np.random.default_rng(n)
    Y, theta, dx, cls = c['Y'].copy(), c['theta'].copy(), c['dx'].copy(), c['cls'].copy()
    refs = pose_ref.smooth_refs(n, K, C, seed=n)
    M = 12                                                               # planted: images of the references at nearby poses
    for i in range(M):
        cls[i] = (0, 1, 3)[i % 3]
    cls[5] = -1                                                          # (stays skipped)
    th_true = rng.uniform(-np.pi, np.pi, M).astype(F32)
    dx_true = (rng.uniform(-0.12, 0.12, (M, 2)) / t).astype(F32)
    Y[:M] = (pose_ref.render(refs, cls[:M], th_true, dx_true, t) + 0.05 * rng.standard_normal((M, C, n, n))).astype(F32)
    theta[:M] = (th_true + rng.uniform(-0.04, 0.04, M)).astype(F32)
    dx[:M] = (dx_true + rng.uniform(-0.7, 0.7, (M, 2)) * 2 / (n - 1) / t).astype(F32)
    from tvae import _cluster_lib as CL
    dY, dth, ddx, dcls, dref = _dev(Y), _dev(theta), _dev(dx), _dev(cls, torch.int32), _dev(refs)
    st = new_gpu_state(N)
    mom_try = torch.full((N, 15), SENT_F, device=DEV)
    exact_checked = near = accepted = rejected = 0
    for it in range(ITERATIONS + 1):
        first = it == 0
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_pose_moments', dY, dth if first else st['theta_try'], ddx if first else st['dx_try'], dcls, dref,
                    mom_try, N, C, n, K, t, c['radius'], c['edge'])
        before = host_state(st) if not first else polish_ref.new_state(N)
        steps0, ended0 = before['steps'].copy(), before['ended'].copy()     # (polish_ref.step changes `before` in place)
        run_step(st, dcls, dth, ddx, mom_try, n, K, first, t)
        want = polish_ref.step(before, mom_try.cpu().numpy(), cls, K, theta, dx, n, t, MAX_SHIFT, MAX_ANGLE, first)
        got = host_state(st)
        for k in ('steps', 'ended'):
            assert np.array_equal(got[k], want[k]), (it, k, np.flatnonzero(got[k] != want[k]))
        assert np.array_equal(got['lam'].view(np.int64), want['lam'].view(np.int64)), it
        for k in ('theta', 'dx', 'score'):
            assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (it, k)
        assert np.array_equal(got['mom'], want['mom'].astype(np.float64))
        if not first:
            accepted += int((got['steps'] > steps0).sum())
            rejected += int(((got['steps'] == steps0) & (ended0 == 0)).sum())
        for i in range(N):
            g3 = (got['theta_try'][i], got['dx_try'][i, 0], got['dx_try'][i, 1])
            w3 = (want['theta_try'][i], want['dx_try'][i, 0], want['dx_try'][i, 1])
            ex = want['exact'][i]
            if ex is None:                                               # no step, or an image that had ended before
                assert polish_ref.same_bits(g3, w3), (it, i)
                continue
            for g1, w1, e1 in zip(g3, w3, ex):
                if _far_from_a_boundary(e1):
                    assert F32(g1).view(np.int32) == F32(w1).view(np.int32), (it, i, g1, w1, e1)
                    exact_checked += 1
                else:
                    assert _ulps(g1, w1) <= 1, (it, i, g1, w1, e1)
                    near += 1
    print(f'polish_step n={n}: {exact_checked} trial components identical in bits, {near} near a rounding boundary (within an fp32 '
          f'step), {accepted} accepted and {rejected} rejected trials')
    assert exact_checked > 20 * near and accepted >= 2 * (M - 1) and rejected > 0
    final = host_state(st)
    alone = list(HOSTILE) + list(SKIPPED)
    assert np.array_equal(final['theta'][alone].view(np.int32), theta[alone].view(np.int32))
    assert np.array_equal(final['dx'][alone].view(np.int32), dx[alone].view(np.int32))
    assert not final['score'][alone].any() and not final['steps'][alone].any() and final['ended'][alone].all()
    assert (final['score'][:, 1] >= final['score'][:, 0]).all()
    for v in final.values():
        if isinstance(v, np.ndarray):
            assert not (v == (SENT_I if v.dtype == np.int32 else SENT_F)).any()
    # the Python API is this loop, bit for bit
    from tvae import polish
    with guardband.GuardedCalls(replay=True):
        api = polish.polish_poses(dY, dth.view(-1, 1), ddx, cls.copy(), dref, t, ITERATIONS, MAX_SHIFT, MAX_ANGLE,
                                  c['radius'] if masked else None, c['edge'])
    for v, k in zip(api, ('theta', 'dx', 'score', 'steps')):
        assert np.array_equal(v.cpu().numpy().view(np.int32), final[k].view(np.int32)), k
    assert api[3].dtype == torch.int32 and api[0].shape == (N,) and api[2].shape == (N, 2)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def off_grid(n):
    """The noise-free planted case of test_polish_cpu.py."""
    p = pose_ref.planted(n=n, N=48)
    rng = np.random.default_rng(1000 + n)
    th0 = (p['theta_true'] + rng.uniform(-0.04, 0.04, 48)).astype(F32)
    dx0 = (p['dx_true'] + rng.uniform(-0.7, 0.7, (48, 2)) * 2 / (n - 1)).astype(F32)
    return p, th0, dx0


def _polish(p, th0, dx0, sl=slice(None), refs=None, cls=None, **kw):
    from tvae import polish
    refs = p['refs'] if refs is None else refs
    cls = p['cls'] if cls is None else cls
    with guardband.GuardedCalls(replay=True):
        out = polish.polish_poses(_dev(p['Y'][sl]), _dev(th0[sl]), _dev(dx0[sl]), cls[sl].copy(), _dev(refs), 1.0, ITERATIONS,
                                  MAX_SHIFT, MAX_ANGLE, **kw)
    return [v.cpu().numpy() for v in out]


@pytest.mark.parametrize('n', [32, 64])
def test_planted_poses_are_recovered_end_to_end(n):
    """Every image ends within its own start error / 50 of the planted shift (at most 0.014 px for a 0.7 px start): two orders
    above the fp32 position uncertainty delta (5e-5 to 2e-4 px) and twenty times below the half-pixel quantisation this removes.
    The angle gets the same factor on the case's start error (0.04 rad: 8e-4 rad), not on the image's own: a start angle is
    often within 0.005 rad of the truth, and a fiftieth of that is below what the fp32 sums resolve.  The acceptance compares
    two scores whose three sums each carry an fp32 rounding, nu = 6 * 2^-24 in all, and near the optimum 1 - score =
    (dtheta^2 / 2) DD / PP, so steps below sqrt(2 nu PP / DD) are accepted or rejected by rounding: with PP / DD about 0.25
    on these blobs that is 4e-4 rad (measured: 3.3e-4 rad at n = 64 on the one image of 96 that stalled; the rest end below
    1e-6)."""
    p, th0, dx0 = off_grid(n)
    th, dx, score, steps = _polish(p, th0, dx0)
    half = (n - 1) / 2
    s0 = np.abs(dx0.astype(np.float64) - p['dx_true']).max(1) * half
    s1 = np.abs(dx.astype(np.float64) - p['dx_true']).max(1) * half
    a0 = np.abs(th0.astype(np.float64) - p['theta_true'])
    a1 = np.abs(th.astype(np.float64) - p['theta_true'])
    print(f'polish_poses n={n}: shift error {s0.max():.3f} -> {s1.max():.3e} px, angle error {a0.max():.3f} -> {a1.max():.3e} rad, '
          f'accepted steps {steps.min()} .. {steps.max()}, worst (final / start) shift {np.max(s1 / s0):.3e} angle {np.max(a1 / a0):.3e}')
    assert (s1 <= s0 / 50).all() and (a1 <= a0.max() / 50).all()
    assert (score[:, 1] >= score[:, 0]).all() and (score[:, 1] > 1 - 1e-5).all()
    ra, rd, _ = polish_ref.radii(n, 1.0, MAX_SHIFT, MAX_ANGLE)
    assert (np.abs(th.astype(np.float64) - th0) <= ra).all() and (np.abs(dx.astype(np.float64) - dx0) <= rd).all()


# ---- 4. invariances ---------------------------------------------------------------------------------------------------------------
def test_reproducible_and_independent_of_the_other_images_and_of_K():
    p, th0, dx0 = off_grid(32)
    full = _polish(p, th0, dx0, mask_radius=0.4 * 32, mask_edge=3.0)
    again = _polish(p, th0, dx0, mask_radius=0.4 * 32, mask_edge=3.0)
    part = _polish(p, th0, dx0, slice(7, 29), mask_radius=0.4 * 32, mask_edge=3.0)
    more = _polish(p, th0, dx0, refs=np.concatenate([p['refs'], np.ones((5,) + p['refs'].shape[1:], F32)]), mask_radius=0.4 * 32,
                   mask_edge=3.0)
    for a, b, c_, d in zip(full, again, part, more):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
        assert np.array_equal(a[7:29].view(np.int32), c_.view(np.int32))
        assert np.array_equal(a.view(np.int32), d.view(np.int32))
    assert full[3].sum() > 48
    # the moments alone: a slice, K + 5 references, the same call again
    c = case(17, 2, N_IMG, True)
    args = (c['t'], c['radius'], c['edge'])
    sub = np.array([19, 3, 4, 9, 16, 0, 22])
    part = run_moments(c['Y'][sub], c['theta'][sub], c['dx'][sub], c['cls'][sub], c['refs'], *args)
    more = run_moments(c['Y'], c['theta'], c['dx'], np.where(c['cls'] == 7, 9, c['cls']),
                       np.concatenate([c['refs'], np.ones((5,) + c['refs'].shape[1:], F32)]), *args)
    again = run_moments(c['Y'], c['theta'], c['dx'], c['cls'], c['refs'], *args)
    assert np.array_equal(part.view(np.int32), c['got'][sub].view(np.int32))
    assert np.array_equal(more.view(np.int32), c['got'].view(np.int32))
    assert np.array_equal(again.view(np.int32), c['got'].view(np.int32))


def test_skipped_and_hostile_images_are_left_alone():
    from tvae import polish
    c = case(32, 3, N_IMG, False)
    alone = list(HOSTILE) + list(SKIPPED)
    with guardband.GuardedCalls(replay=True):
        th, dx, score, steps = (v.cpu().numpy() for v in polish.polish_poses(
            _dev(c['Y']), _dev(c['theta']), _dev(c['dx']), c['cls'].copy(), _dev(c['refs']), c['t'], 3))
    assert np.array_equal(th[alone].view(np.int32), c['theta'][alone].view(np.int32))
    assert np.array_equal(dx[alone].view(np.int32), c['dx'][alone].view(np.int32))
    assert not score[alone].any() and not steps[alone].any()
    assert not c['got'][list(SKIPPED)].any() and not c['got'][list(HOSTILE), :14].any() and (c['got'][list(HOSTILE), 14] > 0).all()
    assert (score[:, 1] >= score[:, 0]).all() and np.isfinite(score).all()
    # every reference NaN: nothing of ref is read for a skipped image; the empty class's reference NaN: nothing changes
    nan = run_moments(c['Y'], c['theta'], c['dx'], c['cls'], np.full_like(c['refs'], np.nan), c['t'])
    assert not nan[list(SKIPPED)].any()
    refs = c['refs'].copy()
    refs[2] = np.nan
    assert (c['cls'] != 2).all()
    other = run_moments(c['Y'], c['theta'], c['dx'], c['cls'], refs, c['t'])
    assert np.array_equal(other.view(np.int32), c['got'].view(np.int32))


# ---- 5. rejection -----------------------------------------------------------------------------------------------------------------
def test_unsupported_arguments_are_rejected_and_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    N, C, n, K = 4, 1, 8, 2
    Y, refs = torch.zeros(N, 17, n, n, device=DEV), torch.zeros(K, 17, n, n, device=DEV)
    big = torch.zeros(1, 1, 129, 129, device=DEV)
    th, dx = torch.zeros(N, device=DEV), torch.zeros(N, 2, device=DEV)
    cls = torch.zeros(N, dtype=torch.int32, device=DEV)
    mom = torch.full((N, 15), SENT_F, device=DEV)

    def moments(Y=Y, th=th, dx=dx, cls=cls, refs=refs, mom=mom, N=N, C=C, n=n, K=K, t=1.0, radius=0.0, edge=0.0):
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():                               # a rejected call must leave every tensor as it was
                CL.call('tvae_pose_moments', Y, th, dx, cls, refs, mom, N, C, n, K, t, radius, edge)

    for kw in (dict(n=129, Y=big, refs=big, N=1), dict(C=17), dict(K=0), dict(K=65536), dict(t=0.0), dict(t=-1.0),
               dict(t=float('nan')), dict(t=float('inf')), dict(edge=-1.0), dict(edge=float('inf')), dict(edge=float('nan')),
               dict(radius=float('nan')), dict(radius=float('inf')), dict(mom=th), dict(mom=None), dict(Y=None), dict(refs=None),
               dict(cls=None), dict(n=1), dict(N=0), dict(C=0)):
        moments(**kw)
    flat = torch.full((N * 15 + 2 * N,), SENT_F, device=DEV)            # an output that overlaps an input
    with pytest.raises(TvaeHipError):
        with guardband.GuardedCalls():
            CL.call('tvae_pose_moments', Y, th, flat[N * 15 - 4:N * 15 - 4 + 2 * N].view(N, 2), cls, refs, flat[:N * 15].view(N, 15),
                    N, C, n, K, 1.0, 0.0, 0.0)
    assert (mom == SENT_F).all() and (flat == SENT_F).all()

    st = new_gpu_state(N)
    mt = torch.zeros(N, 15, device=DEV)

    def step(N=N, n=n, K=K, t=1.0, shift=1.0, angle=0.05, cls=cls, th0=th, mt=mt, **repl):
        s = dict(st, **repl)
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():
                CL.call('tvae_pose_polish_step', cls, th0, dx, mt, *(s[k] for k in STATE), N, n, K, 1, t, shift, angle)

    for kw in (dict(n=129), dict(n=1), dict(K=0), dict(K=65536), dict(N=0), dict(t=0.0), dict(t=-2.0), dict(t=float('nan')),
               dict(shift=-1.0), dict(shift=float('nan')), dict(angle=-0.1), dict(angle=float('inf')), dict(theta=th),
               dict(theta_try=None), dict(lam=None), dict(ended=None), dict(cls=None), dict(mt=None), dict(mom=mt),
               dict(steps=st['ended'])):
        step(**kw)
    for k, v in st.items():
        assert (v == (SENT_I if v.dtype == torch.int32 else SENT_F)).all(), k
    # and the Python API says what is wrong before anything is launched
    from tvae import polish
    with pytest.raises(TvaeHipError, match='Fourier-downsample'):
        polish.polish_poses(big, th[:1], dx[:1], cls[:1], big)
    Y1, R1 = torch.zeros(N, 1, n, n, device=DEV), torch.zeros(K, 1, n, n, device=DEV)
    with pytest.raises(TvaeHipError, match='t_scale'):
        polish.polish_poses(Y1, th, dx, cls, R1, t_scale=0.0)
    with pytest.raises(TvaeHipError, match='max_shift'):
        polish.polish_poses(Y1, th, dx, cls, R1, max_shift=-1.0)


# ---- 6. the command line --------------------------------------------------------------------------------------------------------------
def test_polish_poses_py_writes_its_files_and_equals_the_library_call(tmp_path):
    from tvae import align, polish
    p = pose_ref.planted(seed=31, N=6, n=16, K=2)
    rng = np.random.default_rng(32)
    rot = (p['theta_true'] + rng.uniform(-0.03, 0.03, 6)).astype(F32).reshape(6, 1)
    tr = (p['dx_true'] + rng.uniform(-0.6, 0.6, (6, 2)) * 2 / 15).astype(F32)
    np.save(tmp_path / 'stack.npy', p['Y'][:, 0])
    np.save(tmp_path / 'rotations.npy', rot)
    np.save(tmp_path / 'translations.npy', tr)
    np.save(tmp_path / 'clusters.npy', p['cls'])
    cmd = [sys.executable, os.path.join(PKG, 'polish_poses.py'), '--stack', str(tmp_path / 'stack.npy'), '--clusters',
           str(tmp_path / 'clusters.npy'), '--n-clusters', '2', '--rotations', str(tmp_path / 'rotations.npy'), '--translations',
           str(tmp_path / 'translations.npy'), '--out-dir', str(tmp_path / 'out'), '--iterations', '5', '--max-shift', '0.9',
           '--max-angle', '2.5']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / 'out'
    files = ['class_averages_polished.npy', 'polish_scores.npy', 'polish_steps.npy', 'rotations_polished.npy',
             'translations_polished.npy']
    assert sorted(os.listdir(out)) in (files, sorted(files + ['class_averages_polished.jpg']))
    lines = [ln for ln in r.stdout.splitlines() if not ln.startswith('#')]
    assert len(lines) == 2 and all(ln.count('->') == 2 for ln in lines)  # one line per class: both resolutions before -> after
    got_rot, got_tr = np.load(out / 'rotations_polished.npy'), np.load(out / 'translations_polished.npy')
    sc, st = np.load(out / 'polish_scores.npy'), np.load(out / 'polish_steps.npy')
    assert got_rot.shape == (6, 1) and got_rot.dtype == F32 and got_tr.shape == (6, 2) and got_tr.dtype == F32
    assert sc.shape == (6, 2) and sc.dtype == F32 and st.shape == (6,) and st.dtype == np.int32
    avg = np.load(out / 'class_averages_polished.npy')
    assert avg.shape == (2, 1, 16, 16) and avg.dtype == F32
    Y, th0, d0 = _dev(p['Y']), _dev(rot.reshape(-1)), _dev(tr)
    refs = align.class_averages(Y, th0, d0, p['cls'], 2, 1.0)[0]
    th, d, sc2, st2 = polish.polish_poses(Y, th0, d0, p['cls'], refs, 1.0, 5, 0.9, np.radians(2.5))
    assert np.array_equal(th.cpu().numpy().view(np.int32), got_rot.reshape(-1).view(np.int32))
    assert np.array_equal(d.cpu().numpy().view(np.int32), got_tr.view(np.int32))
    assert np.array_equal(sc2.cpu().numpy().view(np.int32), sc.view(np.int32)) and np.array_equal(st2.cpu().numpy(), st)
    assert np.array_equal(align.class_averages(Y, th, d, p['cls'], 2, 1.0)[0].cpu().numpy(), avg)
    assert st.sum() > 0 and (sc[:, 1] >= sc[:, 0]).all()
