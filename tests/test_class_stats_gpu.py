"""Half sets, variance maps and the ring correlation of the class averages on the GPU: tvae_class_halves and tvae_class_frc
behind their C ABI (every call under guard bands with replay, outputs and workspaces filled with a sentinel), tvae.align
against the fp64 restatement tests/frc_ref.py, and the TVAE_CLASS_FRC switch of the clustering command line with
class_resolution.py.  Inputs, poses, labels, the fp64 aligned images and their bounds are those of test_align_gpu.py.

Tolerances against fp64.  avg and the halves: average_bounds of test_align_gpu.py on the member list in question (the mean
of the members' sampling bounds plus cnt 2^-24 mean |A| for the sums; the kernel adds at most 16 terms in fp32 and the
rest in fp64, which is within that).  Variance, (Q - S^2 / m) / (m - 1) with Q = sum A^2 and S = sum A over the m members:
    dQ <= sum_i (2 |A_i| b_i + b_i^2) + 33 * 2^-24 * sum A_i^2      (b_i: the sampling bound of image i; a chunk sum of 32
    dS <= sum_i b_i + 33 * 2^-24 * sum |A_i|                         squares or samples in fp32, fp64 above it)
    |var - ref| <= (dQ + (2 |S| dS + dS^2) / m) / (m - 1)
The ring correlation: frc_ref.frc_bounds (a coefficient within (2 n + 16) 2^-24 sum |a m| of the exact one), the three sums
within those bounds and frc within 3 bound / sqrt(P0 P1), where the test requires bound / sqrt(P0 P1) <= 1e-2 of every ring
of every plane it compares.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref
import frc_ref
import guardband
import test_align_gpu as TA
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

DEV = TA.DEV
EPS = TA.EPS
SENT_F, SENT_I = TA.SENT_F, -77
N_IMG, K_CLS = TA.N_IMG, TA.K_CLS
GEOMETRIES = TA.GEOMETRIES
FRC_SIDES = (5, 16, 33, 65)


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


_dev = TA._dev


# ---- the C ABI under guard bands ---------------------------------------------------------------------------------------------
def run_halves(Y, theta, dx, order, seg, t, N=None):
    """tvae_class_halves with sentinel-filled outputs and workspace -> numpy (avg, halves, var, counts)."""
    from tvae import _cluster_lib as CL
    _, C, n, _ = Y.shape
    N = Y.shape[0] if N is None else N
    K = len(seg) - 1
    wsf = CL.query('tvae_class_halves_ws_floats', N, K, C, n)
    assert wsf > 0
    ws = torch.full((wsf,), SENT_F, device=DEV)
    avg = torch.full((K, C, n, n), SENT_F, device=DEV)
    half = torch.full((2, K, C, n, n), SENT_F, device=DEV)
    var = torch.full((K, C, n, n), SENT_F, device=DEV)
    counts = torch.full((K, 2), SENT_I, dtype=torch.int32, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_class_halves', _dev(Y), _dev(theta), _dev(dx), _dev(order, torch.int32), _dev(seg, torch.int32), avg,
                half, var, counts, ws, wsf, N, C, n, K, t)
    out = avg.cpu().numpy(), half.cpu().numpy(), var.cpu().numpy(), counts.cpu().numpy()
    assert not any((o == SENT_F).any() for o in out[:3]) and not (out[3] == SENT_I).any()
    return out


def run_frc(a, b, radius=0.0, edge=0.0):
    """tvae_class_frc on a[P][n][n], b[P][n][n] with sentinel-filled outputs and workspace -> numpy (frc, sums)."""
    from tvae import _cluster_lib as CL
    P, n, _ = a.shape
    R = CL.query('tvae_frc_rings', n)
    wsf = CL.query('tvae_class_frc_ws_floats', P, n)
    assert R == n // 2 + 1 and wsf > 0
    ws = torch.full((wsf,), SENT_F, device=DEV)
    curve = torch.full((P, R), SENT_F, device=DEV)
    sums = torch.full((P, R, 3), float(SENT_F), dtype=torch.float64, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_class_frc', _dev(a), _dev(b), curve, sums, ws, wsf, P, n, radius, edge)
    return curve.cpu().numpy(), sums.cpu().numpy()


# ---- references and bounds ---------------------------------------------------------------------------------------------------
def half_bounds(ref_aligned, bounds, order, seg, N=N_IMG):
    """average_bounds applied to each half's member list -> [2][K][C][n][n]."""
    lists = frc_ref.half_lists(order, seg, N)
    out = []
    for h in range(2):
        oh, sh = frc_ref.as_segments([pair[h] for pair in lists])
        out.append(TA.average_bounds(ref_aligned, bounds, oh, sh))
    return np.stack(out)


def var_bounds(ref_aligned, bounds, order, seg, N=N_IMG):
    """The module docstring's bound of the variance -> [K][C][n][n]."""
    out = np.zeros((len(seg) - 1,) + ref_aligned.shape[1:])
    for k, pair in enumerate(frc_ref.half_lists(order, seg, N)):
        m = np.concatenate(pair)
        if m.size < 2:
            continue
        A, b = ref_aligned[m], bounds[m][:, None, None, None]
        dQ = (2 * np.abs(A) * b + b * b).sum(0) + 33 * EPS * (A * A).sum(0)
        dS = b.sum() + 33 * EPS * np.abs(A).sum(0)
        out[k] = (dQ + (2 * np.abs(A.sum(0)) * dS + dS * dS) / m.size) / (m.size - 1)
    return out


@functools.lru_cache(maxsize=None)
def case(n, C):
    """The case of test_align_gpu.py (inputs, fp64 aligned images, bounds, the tvae_class_average result) with the fp64
    halves and the guarded tvae_class_halves result added."""
    c = dict(TA.case(n, C))
    c['ref_h'] = frc_ref.class_halves(c['ref'], c['order'], c['seg'])
    c['got_h'] = run_halves(c['Y'], c['theta'], c['dx'], c['order'], c['seg'], c['t'])
    for v in c['ref_h'] + c['got_h']:
        v.setflags(write=False)
    return c


def check_halves(got, ref_aligned, bounds, order, seg, what, N=N_IMG):
    """avg, both halves, the variance and the counts of `got` against fp64 within the bounds; prints the worst figures."""
    avg, half, var, counts = got
    r_avg, r_half, r_var, r_counts = frc_ref.class_halves(ref_aligned, order, seg, N)
    assert counts.tolist() == r_counts.tolist()
    for name, g, r, b in (('avg', avg, r_avg, TA.average_bounds(ref_aligned, bounds, order, seg)),
                          ('halves', half, r_half, half_bounds(ref_aligned, bounds, order, seg, N)),
                          ('var', var, r_var, var_bounds(ref_aligned, bounds, order, seg, N))):
        err = np.abs(g - r)
        live = b > 0
        print(f'{what} {name}: worst error {err.max():.3e}, worst error / bound '
              f'{(err[live] / b[live]).max() if live.any() else 0.0:.3f}')
        assert np.isfinite(g).all() and (err <= b).all(), (name, float(err.max()))
    return r_counts


# ---- halves and variance against fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C', GEOMETRIES)
def test_halves_and_variance_against_fp64(n, C):
    c = case(n, C)
    counts = check_halves(c['got_h'], c['ref'], c['bounds'], c['order'], c['seg'], f'class_halves n={n} C={C} t={c["t"]}')
    assert counts.tolist() == [[150, 150], [1, 0], [0, 0], [30, 30], [20, 19]]
    assert c['got_h'][2][0].max() > 0.1                                  # (unit-variance images: the variance is not trivial)


@pytest.mark.parametrize('n,C', GEOMETRIES)
def test_empty_class_and_class_of_one(n, C):
    c = case(n, C)
    avg, half, var, _ = c['got_h']
    assert not avg[2].any() and not half[:, 2].any() and not var[2].any()            # the empty class: zeros everywhere
    member = c['order'][c['seg'][1]]
    assert np.array_equal(half[0, 1], c['got'][member]) and np.array_equal(avg[1], c['got'][member])
    assert not half[1, 1].any() and not var[1].any()                                 # its half 1 is empty, one member: no variance


# ---- behaviour of tvae_class_halves -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C', GEOMETRIES)
def test_avg_against_class_average(n, C):
    """Both are within average_bounds of the exact mean, hence within the sum of both bounds of each other; not bitwise,
    the order of addition differs."""
    c = case(n, C)
    err = np.abs(c['got_h'][0].astype(np.float64) - c['got_avg'])
    print(f'avg against tvae_class_average n={n} C={C}: worst difference {err.max():.3e}')
    assert (err <= 2 * c['avg_bounds']).all()


@pytest.mark.parametrize('n,C', GEOMETRIES)
def test_halves_against_class_average_on_split_labels(n, C):
    """tvae_class_average on the labels 2 k + parity of the position in the class computes the halves its own way."""
    c = case(n, C)
    lists = frc_ref.half_lists(c['order'], c['seg'], N_IMG)
    order2, seg2 = frc_ref.as_segments([pair[h] for pair in lists for h in range(2)])
    pad = np.setdiff1d(np.arange(N_IMG), order2)                         # (none here: every image has a class)
    assert pad.size == 0 and seg2[-1] == N_IMG
    split = TA.run_average(c['Y'], c['theta'], c['dx'], order2, seg2, c['t'])        # [2 K][C][n][n], class 2 k + h
    split = np.moveaxis(split.reshape((K_CLS, 2) + split.shape[1:]), 1, 0)
    b = half_bounds(c['ref'], c['bounds'], c['order'], c['seg'])
    err = np.abs(c['got_h'][1].astype(np.float64) - split)
    print(f'halves against tvae_class_average on 2K labels n={n} C={C}: worst difference {err.max():.3e}')
    assert (err <= 2 * b).all()


def test_hostile_poses_contribute_exact_zeros():
    n, C, t = 16, 3, 1.0
    c = case(n, 1)
    rng = np.random.default_rng(77)
    Y = rng.standard_normal((N_IMG, C, n, n)).astype(np.float32)
    theta, dx = c['theta'].copy(), c['dx'].copy()
    hostile = np.array([20, 21, 22, 23, 24, 25, 399])
    theta[20] = np.nan
    dx[21], dx[22], dx[23] = (1e30, 0.0), (0.0, np.inf), (np.nan, 0.1)
    dx[24], dx[25], dx[399] = (-np.inf, np.inf), (-1e30, 1e30), (np.nan, np.nan)
    theta[399] = np.inf
    ref = align_ref.align_stack(Y, theta, dx, t)
    assert not ref[hostile].any()
    bounds = TA.image_bounds(Y, dx, t, hostile)
    got = run_halves(Y, theta, dx, c['order'], c['seg'], t)
    check_halves(got, ref, bounds, c['order'], c['seg'], 'hostile poses')           # finite, and b = 0 for the hostile ones
    # a class of hostile members only: they count, and every output is an exact zero
    order, seg = np.array([20, 21, 22, 23, 24, 25, 399]), np.array([0, 7])
    avg, half, var, counts = run_halves(Y, theta, dx, order, seg, t)
    assert counts.tolist() == [[4, 3]] and not avg.any() and not half.any() and not var.any()


def test_hostile_order_entries_are_skipped_and_keep_their_position():
    n, C = 16, 1
    c = case(n, C)
    order = c['order'].copy()
    bad = [0, 5, 31, 32, 150, 299, 300, 301, 399]
    order[bad] = [-1, N_IMG, -1, N_IMG, -(1 << 31), (1 << 31) - 1, -1, N_IMG + 1, N_IMG]
    got = run_halves(c['Y'], c['theta'], c['dx'], order, c['seg'], c['t'])
    counts = check_halves(got, c['ref'], c['bounds'], order, c['seg'], 'hostile order')
    # class 0 loses the even positions 0, 32, 150 and the odd ones 5, 31, 299: the others keep their parity
    assert counts.tolist() == [[147, 147], [0, 0], [0, 0], [29, 30], [19, 19]]
    # had the skipped entries given up their position, position 1 would have moved to half 0
    first = c['order'][1]
    lists = frc_ref.half_lists(order, c['seg'], N_IMG)
    assert first == lists[0][1][0] and first not in lists[0][0]
    assert not got[0][1].any() and not got[1][:, 1].any()                # its only member skipped: an empty class


def test_hostile_seg_is_clamped_on_the_device():
    n, C = 16, 1
    c = case(n, C)
    seg = np.array([-7, 120, 100, -5, 390, N_IMG + 1000])
    clean = np.array([0, 120, 120, 120, 390, N_IMG])
    got = run_halves(c['Y'], c['theta'], c['dx'], c['order'], seg, c['t'])
    want = run_halves(c['Y'], c['theta'], c['dx'], c['order'], clean, c['t'])
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    check_halves(got, c['ref'], c['bounds'], c['order'], clean, 'hostile seg')


def test_a_class_does_not_depend_on_the_others():
    """The same bits with K = 1 on the class's own member list, whatever the class's place in `order`."""
    c = case(16, 3)
    base = c['got_h']
    for k in range(K_CLS):
        members = c['order'][c['seg'][k]:c['seg'][k + 1]]
        if members.size == 0:
            continue
        alone = run_halves(c['Y'], c['theta'], c['dx'], members, np.array([0, members.size]), c['t'])
        assert np.array_equal(alone[0][0], base[0][k]) and np.array_equal(alone[1][:, 0], base[1][:, k]), k
        assert np.array_equal(alone[2][0], base[2][k]) and alone[3][0].tolist() == base[3][k].tolist(), k
    # more classes appended: K changes, the first five do not
    order, seg, _ = align_ref.segments(c['labels'], K_CLS + 3)
    more = run_halves(c['Y'], c['theta'], c['dx'], order, seg, c['t'])
    assert np.array_equal(more[0][:K_CLS], base[0]) and np.array_equal(more[1][:, :K_CLS], base[1])
    assert np.array_equal(more[2][:K_CLS], base[2]) and not more[0][K_CLS:].any() and not more[3][K_CLS:].any()


def test_unsupported_arguments_are_rejected_and_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    Y = torch.zeros(4, 1, 8, 8, device=DEV)
    th, dx = torch.zeros(4, device=DEV), torch.zeros(4, 2, device=DEV)
    order = torch.arange(4, dtype=torch.int32, device=DEV)
    seg = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    avg, var = torch.full((2, 1, 8, 8), SENT_F, device=DEV), torch.full((2, 1, 8, 8), SENT_F, device=DEV)
    half = torch.full((2, 2, 1, 8, 8), SENT_F, device=DEV)
    counts = torch.full((2, 2), SENT_I, dtype=torch.int32, device=DEV)
    wsf = CL.query('tvae_class_halves_ws_floats', 4, 2, 1, 8)
    ws = torch.full((wsf,), SENT_F, device=DEV)
    for N, C, n, K, w in [(4, 1, 8, 0, wsf), (4, 1, 8, 65536, wsf), (4, 1, 1, 2, wsf), (0, 1, 8, 2, wsf), (4, 1, 8, 2, wsf - 1),
                          (4, 0, 8, 2, wsf), (4, 1, 1025, 2, wsf)]:
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():                               # a rejected call must leave every tensor as it was
                CL.call('tvae_class_halves', Y, th, dx, order, seg, avg, half, var, counts, ws, w, N, C, n, K, 1.0)
    assert (avg == SENT_F).all() and (half == SENT_F).all() and (var == SENT_F).all() and (counts == SENT_I).all()
    assert (ws == SENT_F).all()
    a = torch.zeros(3, 8, 8, device=DEV)
    curve = torch.full((3, 5), SENT_F, device=DEV)
    sums = torch.full((3, 5, 3), float(SENT_F), dtype=torch.float64, device=DEV)
    wsf = CL.query('tvae_class_frc_ws_floats', 3, 8)
    ws = torch.full((wsf,), SENT_F, device=DEV)
    inf, nan = float('inf'), float('nan')
    for P, n, w, radius, edge in [(0, 8, wsf, 0.0, 0.0), (65536, 8, wsf, 0.0, 0.0), (3, 1, wsf, 0.0, 0.0), (3, 1025, wsf, 0.0, 0.0),
                                  (3, 8, wsf - 1, 0.0, 0.0), (3, 8, wsf, nan, 0.0), (3, 8, wsf, inf, 1.0), (3, 8, wsf, 2.0, nan),
                                  (3, 8, wsf, 2.0, inf), (3, 8, wsf, 2.0, -1.0), (3, 8, wsf, -inf, 0.0)]:
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():
                CL.call('tvae_class_frc', a, a, curve, sums, ws, w, P, n, radius, edge)
    assert (curve == SENT_F).all() and (sums == SENT_F).all() and (ws == SENT_F).all()


# ---- the ring correlation against fp64 ---------------------------------------------------------------------------------------
def lowpass(rng, n, sigma):
    """A smooth random pattern of unit variance: white noise under a Gaussian envelope exp(-k^2 / (2 sigma^2))."""
    k = np.fft.fftfreq(n) * n
    env = np.exp(-(k[:, None] ** 2 + k[None, :] ** 2) / (2 * sigma * sigma))
    p = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, n))) * env).real
    return p / p.std()


@functools.lru_cache(maxsize=None)
def frc_case(n):
    """24 pairs of planes, the four kinds in turn (plane p is of kind p % 4): the halves of the case above, pure noise
    pairs, a shared low-pass pattern plus independent noise, and the same under the mask (radius 0.35 n, edge 3).  The
    unmasked ones go through one call and the masked ones through another."""
    rng = np.random.default_rng(2900 + n)            # (a draw whose ring 0, the plain sum of a noise plane, is not tiny)
    half = case(n, 3)['got_h'][1]
    live = [(k, ch) for k in (0, 3, 4) for ch in (0, 1)]                 # the classes with members in both halves
    a, b = np.zeros((24, n, n), np.float32), np.zeros((24, n, n), np.float32)
    for p in range(24):
        kind, q = p % 4, p // 4
        if kind == 0:
            a[p], b[p] = half[0][live[q]], half[1][live[q]]
        elif kind == 1:
            a[p], b[p] = rng.standard_normal((2, n, n))
        else:
            shared = 2.0 * lowpass(rng, n, n / 8)
            a[p], b[p] = shared + rng.standard_normal((n, n)), shared + rng.standard_normal((n, n))
    masked = np.arange(24) % 4 == 3
    radius, edge = 0.35 * n, 3.0
    ref = {False: frc_ref.frc(a[~masked], b[~masked]), True: frc_ref.frc(a[masked], b[masked], radius, edge)}
    got = {False: run_frc(a[~masked], b[~masked]), True: run_frc(a[masked], b[masked], radius, edge)}
    d = dict(n=n, a=a, b=b, masked=masked, radius=radius, edge=edge, ref=ref, got=got)
    for v in (a, b) + got[False] + got[True]:
        v.setflags(write=False)
    return d


def check_frc(got, ref, what):
    """The three sums within frc_bounds, frc within 3 bound / sqrt(P0 P1), the condition bound / sqrt(P0 P1) <= 1e-2 on
    every ring of every plane; prints the worst figures."""
    curve, sums = got
    bound = frc_ref.frc_bounds(ref)
    err = np.abs(sums - ref['sums'])
    assert np.isfinite(sums).all() and np.isfinite(curve).all()
    scale = np.sqrt(ref['sums'][..., 1] * ref['sums'][..., 2])
    cond = bound[..., 0] / scale
    ferr = np.abs(curve - ref['frc'])
    print(f'{what}: sums worst error / bound {(err / bound).max():.4f}, frc worst error {ferr.max():.3e}, worst error / '
          f'(3 bound / sqrt(P0 P1)) {(ferr / (3 * cond)).max():.4f}, worst bound / sqrt(P0 P1) {cond.max():.3e}')
    assert (cond <= 1e-2).all(), float(cond.max())
    assert (err <= bound).all(), float((err / bound).max())
    assert (ferr <= 3 * cond).all(), float((ferr / (3 * cond)).max())


@pytest.mark.parametrize('n', FRC_SIDES)
def test_frc_against_fp64(n):
    c = frc_case(n)
    for m in (False, True):
        assert c['got'][m][0].shape == (int(c['masked'].sum()) if m else int((~c['masked']).sum()), n // 2 + 1)
        check_frc(c['got'][m], c['ref'][m], f'class_frc n={n} masked={m}')
    # the shared pattern correlates at low frequency and not at high frequency; pure noise nowhere
    if n >= 33:
        unmasked = np.flatnonzero(~c['masked'])
        lp = c['got'][False][0][unmasked % 4 == 2]
        assert (lp[:, 1:3] > 0.7).all() and np.abs(lp[:, -4:]).mean() < 0.3


# ---- behaviour of tvae_class_frc --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', FRC_SIDES)
def test_identical_and_negated_planes(n):
    c = frc_case(n)
    a = c['a'][~c['masked']]
    ref = frc_ref.frc(a, a)
    same = run_frc(a, a)
    check_frc(same, ref, f'identical planes n={n}')
    cond = frc_ref.frc_bounds(ref)[..., 0] / ref['sums'][..., 1]
    assert (np.abs(same[0] - 1) <= 3 * cond).all()
    neg = run_frc(a, -a)
    check_frc(neg, frc_ref.frc(a, -a), f'negated planes n={n}')
    assert (np.abs(neg[0] + 1) <= 3 * cond).all()


@pytest.mark.parametrize('n', [16, 33])
def test_cosine_plane_has_power_in_ring_five_only(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    a = np.cos(2 * np.pi * (3 * i + 4 * j) / n).astype(np.float32)[None]
    ref = frc_ref.frc(a, a)
    curve, sums = run_frc(a, a)
    bound = frc_ref.frc_bounds(ref)
    assert (np.abs(sums - ref['sums']) <= bound).all()
    others = np.delete(np.arange(n // 2 + 1), 5)
    print(f'cosine n={n}: power in ring 5 {sums[0, 5, 1]:.6e} (n^4 / 2 = {n ** 4 / 2:.6e}), largest elsewhere '
          f'{sums[0, others, 1].max():.3e}')
    assert abs(sums[0, 5, 1] - n ** 4 / 2) <= bound[0, 5, 1] + 1e-6 * n ** 4          # (the fp32 cosine is not the exact one)
    assert (sums[0, others, 1] <= bound[0, others, 1]).all() and sums[0, others, 1].max() < 1e-9 * sums[0, 5, 1]
    assert abs(curve[0, 5] - 1) <= 1e-6


def test_zero_plane_gives_zero_and_nan_stays_in_its_plane():
    n = 33
    c = frc_case(n)
    a, b = c['a'][~c['masked']].copy(), c['b'][~c['masked']].copy()
    base = c['got'][False]
    a[4] = 0.0
    b[9] = 0.0
    a[11, 7, 20] = np.nan
    curve, sums = run_frc(a, b)
    assert not curve[4].any() and not curve[9].any() and not np.isnan(curve[[4, 9]]).any()      # exactly 0, not NaN
    assert not sums[4, :, :2].any() and not sums[9, :, 0].any() and not sums[9, :, 2].any()
    assert np.isnan(curve[11]).all() and np.isnan(sums[11, :, :2]).all()
    assert np.array_equal(sums[11, :, 2], base[1][11, :, 2])                                    # b of that plane is clean
    rest = np.delete(np.arange(a.shape[0]), [4, 9, 11])
    assert np.array_equal(curve[rest], base[0][rest]) and np.array_equal(sums[rest], base[1][rest])


def test_python_frc_on_slices_is_bitwise_the_single_call(monkeypatch):
    from tvae import _cluster_lib as CL, align
    n = 33
    c = frc_case(n)
    a, b = _dev(c['a'][c['masked']]), _dev(c['b'][c['masked']])
    calls = []
    old = CL.call
    monkeypatch.setattr(CL, 'call', lambda name, *args: (calls.append(args[6]), old(name, *args))[1])
    with guardband.GuardedCalls(replay=True):
        whole = align.frc(a, b, c['radius'], c['edge'])
        monkeypatch.setattr(align, 'FRC_WS_FLOATS', 2 * CL.query('tvae_class_frc_ws_floats', 1, n) + 5)
        sliced = align.frc(a.view(2, 3, n, n), b.view(2, 3, n, n), c['radius'], c['edge'])
    assert calls == [6, 2, 2, 2]
    assert sliced[0].shape == (2, 3, n // 2 + 1) and sliced[1].shape == (2, 3, n // 2 + 1, 3)
    assert sliced[0].dtype == torch.float32 and sliced[1].dtype == torch.float64
    assert torch.equal(sliced[0].view(6, -1), whole[0]) and torch.equal(sliced[1].view(6, -1, 3), whole[1])
    assert np.array_equal(whole[0].cpu().numpy(), c['got'][True][0]) and np.array_equal(whole[1].cpu().numpy(), c['got'][True][1])


def test_python_api_is_bitwise_the_c_abi_and_reproducible():
    from tvae import align
    c = case(33, 3)
    Y, th, dx = _dev(c['Y']), _dev(c['theta']).view(-1, 1), _dev(c['dx'])
    with guardband.GuardedCalls(replay=True):
        r1 = align.class_halves(Y, th, dx, c['labels'].copy(), K_CLS, c['t'])
        r2 = align.class_halves(Y, th, dx, torch.from_numpy(c['labels'].copy()).to(DEV), None, c['t'])
        f1 = align.frc(r1[1][0], r1[1][1])
        f2 = align.frc(r2[1][0], r2[1][1], None, 0.0)
    for g, w in zip(r1, c['got_h']):
        assert np.array_equal(g.cpu().numpy(), w)
    assert all(torch.equal(x, y) for x, y in zip(r1, r2)) and all(torch.equal(x, y) for x, y in zip(f1, f2))
    assert r1[1].shape == (2, K_CLS, 3, 33, 33) and r1[3].shape == (K_CLS, 2) and r1[3].dtype == torch.int32
    assert f1[0].shape == (K_CLS, 3, 17) and f1[1].shape == (K_CLS, 3, 17, 3)
    got = run_frc(c['got_h'][1][0].reshape(-1, 33, 33), c['got_h'][1][1].reshape(-1, 33, 33))
    assert np.array_equal(f1[0].cpu().numpy().reshape(-1, 17), got[0]) and np.array_equal(f1[1].cpu().numpy().reshape(-1, 17, 3), got[1])
    assert not f1[0][1].any() and not f1[0][2].any()                     # a class with an empty half: FRC exactly 0


def test_argument_checks():
    from tvae import align
    from tvae._lib import TvaeHipError
    Y, th, dx = torch.zeros(4, 1, 8, 8, device=DEV), torch.zeros(4, device=DEV), torch.zeros(4, 2, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64)
    for bad in [(Y.double(), th, dx), (Y[:, :, :, ::2], th, dx), (Y.view(4, 8, 8), th, dx), (Y, th[:3], dx), (Y, th, dx[:, :1]),
                (Y, th.cpu(), dx), (torch.zeros(4, 1, 8, 6, device=DEV), th, dx), (torch.zeros(4, 1, 1, 1, device=DEV), th, dx)]:
        with pytest.raises(TvaeHipError):
            align.class_halves(*bad, lab, 2)
    for lab_bad, K in ((lab[:3], 2), (lab, 0), (lab, 65536)):
        with pytest.raises(TvaeHipError):
            align.class_halves(Y, th, dx, lab_bad, K)
    a = torch.zeros(2, 8, 8, device=DEV)
    for bad in [(a, a[:1]), (a.double(), a.double()), (a[:, :, ::2], a[:, :, ::2]), (a[:, :, :6].contiguous(), a[:, :, :6].contiguous()),
                (a, a.cpu()), (torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)), (torch.zeros(1, 1, device=DEV),) * 2]:
        with pytest.raises(TvaeHipError):
            align.frc(*bad)
    for radius, edge in ((float('nan'), 0.0), (3.0, -1.0), (3.0, float('inf'))):
        with pytest.raises(TvaeHipError):
            align.frc(a, a, radius, edge)


# ---- the command lines -------------------------------------------------------------------------------------------------------
def test_clustering_particles_writes_the_class_statistics_and_class_resolution_py_reproduces_them(tmp_path):
    """clustering_particles.py on tests/golden/stack_ref.mrcs (5 images cropped to 6 x 6, MLP encoder, t = 0.1), as the
    class-average command-line test of test_align_gpu.py runs it: with TVAE_CLASS_FRC=1 it adds the class-statistics files,
    unset the directory is what it was."""
    import src.models as M
    from tvae import align, resolution
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
        for name in ('TVAE_CLASS_AVERAGES', 'TVAE_FIGURES', 'TVAE_CLASS_FRC'):
            env.pop(name, None)
        if mode == 'on':
            env['TVAE_CLASS_FRC'] = '1'
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert ('gold-standard' in r.stderr) == (mode == 'on')
        listing[mode] = sorted(os.listdir(tmp_path / mode))
    today = ['clusters.npy', 'latents.npy', 'results.txt', 'rotations.npy', 'translations.npy']
    assert listing['off'] == today
    extra = sorted(set(listing['on']) - set(today))
    files = ['class_counts.npy', 'class_frc.npy', 'class_halves.npy', 'class_resolution.txt', 'class_variance.npy']
    assert extra in (files, sorted(files + ['class_frc.jpg', 'class_variance.jpg']))
    on = tmp_path / 'on'
    for f in today[:2] + today[3:]:
        assert np.array_equal(np.load(on / f), np.load(tmp_path / 'off' / f)), f
    clusters = np.load(on / 'clusters.npy')
    halves, var = np.load(on / 'class_halves.npy'), np.load(on / 'class_variance.npy')
    curve, counts = np.load(on / 'class_frc.npy'), np.load(on / 'class_counts.npy')
    assert halves.shape == (2, 2, 1, 6, 6) and halves.dtype == np.float32 and var.shape == (2, 1, 6, 6)
    assert curve.shape == (2, 1, 4) and curve.dtype == np.float32 and counts.shape == (2, 2)
    assert counts.sum(1).tolist() == np.bincount(clusters, minlength=2).tolist() and counts.sum() == 5
    assert ((counts[:, 0] - counts[:, 1]) >= 0).all() and ((counts[:, 0] - counts[:, 1]) <= 1).all()
    # bitwise tvae.align of the saved pose and label files, and within the bounds of fp64
    Y = torch.from_numpy(align.load_stack(stack, 6)).to(DEV)
    th = torch.from_numpy(np.load(on / 'rotations.npy').astype(np.float32)).to(DEV)
    dx = torch.from_numpy(np.load(on / 'translations.npy').astype(np.float32)).to(DEV)
    t = align.translation_scale('unimodal')
    _, wh, wv, wc = align.class_halves(Y, th, dx, clusters, 2, t)
    assert np.array_equal(wh.cpu().numpy(), halves) and np.array_equal(wv.cpu().numpy(), var) and wc.tolist() == counts.tolist()
    assert resolution.default_mask(6)[0] < 0                             # 6 x 6 images: too small for the default mask, none
    wf, _ = align.frc(wh[0], wh[1], *resolution.default_mask(6))
    assert np.array_equal(wf.cpu().numpy(), curve)
    Yh, dxh = Y.cpu().numpy(), dx.cpu().numpy()
    ref = align_ref.align_stack(Yh, th.cpu().numpy(), dxh, float(np.float32(0.1)))
    order, seg, _ = align_ref.segments(clusters, 2)
    r_half = frc_ref.class_halves(ref, order, seg)[1]
    assert (np.abs(halves - r_half) <= half_bounds(ref, TA.image_bounds(Yh, dxh, 0.1), order, seg, 5)).all()
    # class_resolution.txt: comment lines, then one line per class
    lines = open(on / 'class_resolution.txt').read().splitlines()
    assert any('gold-standard' in ln for ln in lines if ln.startswith('#'))
    rows = [ln.split() for ln in lines if not ln.startswith('#')]
    assert len(rows) == 2 and all(len(r) == 5 for r in rows)
    for k, r in enumerate(rows):
        assert int(r[0]) == k and [int(r[1]), int(r[2])] == counts[k].tolist()
        assert 6 / 3 - 1e-3 <= float(r[3]) <= 6.0 + 1e-3 and 6 / 3 - 1e-3 <= float(r[4]) <= 6.0 + 1e-3       # n / r*, 1 <= r* <= R - 1
        assert float(r[3]) <= float(r[4]) + 1e-9                         # the curve crosses 0.5 no later than 0.143
    # class_resolution.py: the same from the files alone
    cmd = [sys.executable, os.path.join(PKG, 'class_resolution.py'), '--stack', stack, '--crop', '6', '--t-inf', 'unimodal',
           '--rotations', str(on / 'rotations.npy'), '--translations', str(on / 'translations.npy'),
           '--clusters', str(on / 'clusters.npy'), '--out-dir', str(tmp_path / 'again')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    again = tmp_path / 'again'
    for f in ('class_halves.npy', 'class_frc.npy', 'class_variance.npy', 'class_counts.npy'):
        assert np.array_equal(np.load(again / f), np.load(on / f)), f
    assert open(again / 'class_resolution.txt').read() == open(on / 'class_resolution.txt').read()
