"""Aligned images and aligned class averages on the GPU: tvae_align_stack and tvae_class_average behind their C ABI (every
call under guard bands with replay, outputs and workspace filled with a sentinel), tvae.align against the fp64
restatement tests/align_ref.py, and the TVAE_CLASS_AVERAGES switch of the clustering command line with class_averages.py.

Tolerance against fp64 (poses: the fp32 values converted to double).  The bilinear sample with a zero border is a
continuous, piecewise bilinear function of the position; its slope along an axis is at most g_i, the largest difference
between adjacent pixels of the zero-bordered image i.  The fp32 position is about a dozen roundings away from the exact
one (the grid coordinate, two products and two sums per axis, the scale to pixels, the two sincos errors), each relative
to a quantity of size at most 2 + t |dx_i|_inf in coordinate units, that is (n - 1) / 2 times as much in pixels:
    delta_i = 16 * 2^-24 * (2 + t |dx_i|_inf) * (n - 1) / 2            (pixels per axis)
    |A_i - ref| <= 2 g_i delta_i + 4 * 2^-24 * max |y_i|               (two axes; the four roundings of the blend)
A class average: the mean of its members' bounds plus cnt * 2^-24 * mean |A| (the fp32 sum of cnt terms and the division).
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
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 2.0 ** -24
SENT_F = -12345.5
N_IMG, K_CLS = 400, 5
GEOMETRIES = [(n, C) for n in (5, 16, 33, 65) for C in (1, 3)]


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


# ---- the C ABI under guard bands ---------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype).contiguous()


def run_align(Y, theta, dx, t):
    """tvae_align_stack into a sentinel-filled output -> numpy [N][C][n][n]."""
    from tvae import _cluster_lib as CL
    N, C, n, _ = Y.shape
    out = torch.full((N, C, n, n), SENT_F, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_align_stack', _dev(Y), _dev(theta), _dev(dx), out, N, C, n, t)
    return out.cpu().numpy()


def run_average(Y, theta, dx, order, seg, t, N=None):
    """tvae_class_average with sentinel-filled averages and workspace -> numpy [K][C][n][n]."""
    from tvae import _cluster_lib as CL
    _, C, n, _ = Y.shape
    N = Y.shape[0] if N is None else N
    K = len(seg) - 1
    wsf = CL.query('tvae_class_average_ws_floats', N, K, C, n)
    assert wsf > 0
    ws = torch.full((wsf,), SENT_F, device=DEV)
    avg = torch.full((K, C, n, n), SENT_F, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_class_average', _dev(Y), _dev(theta), _dev(dx), _dev(order, torch.int32), _dev(seg, torch.int32), avg,
                ws, wsf, N, C, n, K, t)
    return avg.cpu().numpy()


# ---- inputs, references and bounds -----------------------------------------------------------------------------------------
def make_labels(rng, N=N_IMG):
    """One class of 300 members (several chunks), one of a single member, one empty, two that share the rest."""
    lab = np.concatenate([np.zeros(300, int), np.ones(1, int), np.full(60, 3), np.full(N - 361, 4)])
    return rng.permutation(lab)


def make_poses(rng, n, N=N_IMG):
    """fp32 theta [N], dx [N][2] in coordinate units (before the division by t)."""
    h = 2.0 / (n - 1)
    theta = rng.uniform(-np.pi, np.pi, N)
    dx = rng.uniform(-0.5, 0.5, (N, 2))
    theta[:8] = [0.0, np.pi / 2, -np.pi / 2, np.pi, 7.0, -20.0, 0.0, 0.0]
    dx[:6] = 0.0                                                         # the special angles without a shift
    dx[6], dx[7] = (h, -2 * h), (-3 * h, 0.0)                            # whole pixels, no rotation
    dx[8], dx[9], dx[10] = (2 * h, h), (0.0, -h), (1.5, -1.5)            # whole pixels under a rotation; half out of frame
    dx[11], dx[12], dx[13] = (-1.5, 0.3), (3.0, 0.0), (0.0, -3.0)        # dx = 3: fully out of frame
    dx[14:40] = rng.uniform(-1.5, 1.5, (26, 2))
    return theta.astype(np.float32), dx.astype(np.float32)


def adjacent_step(Y):
    """g_i: the largest difference between adjacent pixels of the zero-bordered image i (every channel)."""
    P = np.pad(np.asarray(Y, dtype=np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    gh = np.abs(np.diff(P, axis=3)).max(axis=(1, 2, 3))
    gv = np.abs(np.diff(P, axis=2)).max(axis=(1, 2, 3))
    return np.maximum(gh, gv)


def image_bounds(Y, dx, t, hostile=None):
    n = Y.shape[-1]
    with np.errstate(invalid='ignore', over='ignore'):
        delta = 16 * EPS * (2 + np.float64(np.float32(t)) * np.abs(dx.astype(np.float64)).max(1)) * (n - 1) / 2
        b = 2 * adjacent_step(Y) * delta + 4 * EPS * np.abs(Y).max(axis=(1, 2, 3))
    if hostile is not None:
        b[hostile] = 0.0                                                 # exact zeros are required there
    assert np.isfinite(b).all()
    return b


def average_bounds(ref_aligned, bounds, order, seg):
    """[K][C][n][n]: mean of the members' bounds + cnt 2^-24 mean |A|."""
    K = len(seg) - 1
    out = np.zeros((K,) + ref_aligned.shape[1:])
    for k in range(K):
        m = np.asarray(order[seg[k]:seg[k + 1]], dtype=np.int64)
        m = m[(m >= 0) & (m < ref_aligned.shape[0])]
        if m.size:
            out[k] = bounds[m].mean() + m.size * EPS * np.abs(ref_aligned[m]).mean(0)
    return out


@functools.lru_cache(maxsize=None)
def case(n, C):
    """Inputs, the fp64 reference (computed once, never modified) and the guarded GPU results of one geometry.  C = 1 runs
    at t = 1; C = 3 at t = 0.1 with the translations scaled by 10, as the unimodal encoder reports them."""
    rng = np.random.default_rng(1000 * n + C)
    t = 1.0 if C == 1 else 0.1
    Y = rng.standard_normal((N_IMG, C, n, n)).astype(np.float32)
    theta, dx = make_poses(rng, n)
    dx = (dx / np.float32(t)).astype(np.float32)
    labels = make_labels(rng)
    order, seg, counts = align_ref.segments(labels, K_CLS)
    t64 = float(np.float32(t))                                           # the factor the kernel gets
    ref = align_ref.align_stack(Y, theta, dx, t64)
    ref_avg, ref_cnt = align_ref.class_averages(ref, order, seg)
    bounds = image_bounds(Y, dx, t)
    d = dict(n=n, C=C, t=t, Y=Y, theta=theta, dx=dx, labels=labels, order=order, seg=seg, counts=counts, ref=ref,
             ref_avg=ref_avg, ref_cnt=ref_cnt, bounds=bounds, avg_bounds=average_bounds(ref, bounds, order, seg),
             got=run_align(Y, theta, dx, t), got_avg=run_average(Y, theta, dx, order, seg, t))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- against fp64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C', GEOMETRIES)
def test_align_stack_against_fp64(n, C):
    c = case(n, C)
    from tvae import _cluster_lib as CL
    chunk = CL.query('tvae_class_average_chunk', N_IMG, K_CLS, C, n)
    assert c['counts'].tolist() == [300, 1, 0, 60, 39] and 300 > 2 * chunk       # the large class spans several chunks
    err = np.abs(c['got'] - c['ref']).max(axis=(1, 2, 3))
    ratio = err / c['bounds']
    print(f'align_stack n={n} C={C} t={c["t"]}: worst error {err.max():.3e}, worst error / bound {ratio.max():.3f}')
    assert not (c['got'] == SENT_F).any()
    assert (err <= c['bounds']).all(), np.flatnonzero(err > c['bounds'])[:10]
    # dx = 3 is fully out of frame: exact zeros
    assert not c['got'][12].any() and not c['got'][13].any() and not c['ref'][12].any() and not c['ref'][13].any()
    # theta = 0 and dx = 0 is the identity, theta = 0 and a whole-pixel shift a shifted copy: exact up to the bound, and
    # partly out of frame images keep a non-trivial part
    assert np.abs(c['got'][0] - c['Y'][0]).max() <= c['bounds'][0]
    assert c['got'][10].any() and (c['got'][10] == 0).any()


@pytest.mark.parametrize('n,C', GEOMETRIES)
def test_class_averages_against_fp64(n, C):
    c = case(n, C)
    err = np.abs(c['got_avg'] - c['ref_avg'])
    live = c['avg_bounds'] > 0
    print(f'class_average n={n} C={C} t={c["t"]}: worst error {err.max():.3e}, worst error / bound '
          f'{(err[live] / c["avg_bounds"][live]).max():.3f}')
    assert not (c['got_avg'] == SENT_F).any()
    assert (err <= c['avg_bounds']).all()
    assert not c['got_avg'][2].any()                                     # the empty class: zeros
    assert np.abs(c['got_avg'][1] - c['ref'][c['order'][c['seg'][1]]]).max() <= c['bounds'].max()   # the class of one


@pytest.mark.parametrize('n,C', GEOMETRIES)
def test_fused_against_plain_form(n, C):
    """class_averages = the per-class mean of align_stack's output within cnt 2^-24 mean |A| per pixel."""
    c = case(n, C)
    A = c['got'].astype(np.float64)
    for k in range(K_CLS):
        m = c['order'][c['seg'][k]:c['seg'][k + 1]]
        if m.size == 0:
            assert not c['got_avg'][k].any()
            continue
        tol = m.size * EPS * np.abs(A[m]).mean(0)
        err = np.abs(c['got_avg'][k] - A[m].mean(0))
        assert (err <= tol).all(), (k, float(err.max()), float(tol.min()))
    assert np.array_equal(c['got_avg'][1], c['got'][c['order'][c['seg'][1]]])        # one member: the aligned image itself


def _aten_matrices(theta, dx, t):
    """affine_grid's x is u0 and its y is -u1: the sampling point (x0, -x1) = (gx c - gy s + t dx0, gx s + gy c - t dx1)."""
    c, s = torch.cos(theta), torch.sin(theta)
    return torch.stack([torch.stack([c, -s, t * dx[:, 0]], 1), torch.stack([s, c, -t * dx[:, 1]], 1)], 1)


@pytest.mark.parametrize('n,C', GEOMETRIES)
def test_align_stack_against_grid_sample(n, C):
    """Both in fp32: each is within the bound of the exact value, so they are within twice the bound of each other."""
    c = case(n, C)
    Y, th, dx = _dev(c['Y']), _dev(c['theta']), _dev(c['dx'])
    grid = torch.nn.functional.affine_grid(_aten_matrices(th, dx, c['t']), list(Y.shape), align_corners=True)
    gs = torch.nn.functional.grid_sample(Y, grid, mode='bilinear', padding_mode='zeros', align_corners=True).cpu().numpy()
    err = np.abs(c['got'].astype(np.float64) - gs).max(axis=(1, 2, 3))
    print(f'grid_sample n={n} C={C}: worst difference / (2 bound) {(err / (2 * c["bounds"])).max():.3f}')
    assert (err <= 2 * c['bounds']).all(), np.flatnonzero(err > 2 * c['bounds'])[:10]


# ---- hostile inputs ----------------------------------------------------------------------------------------------------------
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
    order, seg = c['order'], c['seg']
    ref = align_ref.align_stack(Y, theta, dx, t)
    assert not ref[hostile].any()
    bounds = image_bounds(Y, dx, t, hostile)
    got = run_align(Y, theta, dx, t)                                     # the guard bands are checked in here
    assert not got[hostile].any() and np.isfinite(got).all()
    assert (np.abs(got - ref).max(axis=(1, 2, 3)) <= bounds).all()
    avg = run_average(Y, theta, dx, order, seg, t)
    ref_avg, _ = align_ref.class_averages(ref, order, seg)
    assert np.isfinite(avg).all()
    assert (np.abs(avg - ref_avg) <= average_bounds(ref, bounds, order, seg)).all()


def test_hostile_order_entries_are_skipped():
    n, C = 16, 1
    c = case(n, C)
    order = c['order'].copy()
    seg = c['seg']
    bad = [0, 5, 31, 32, 150, 299, 300, 301, 399]                        # in the large class, the class of one and the others
    order[bad] = [-1, N_IMG, -1, N_IMG, -(1 << 31), (1 << 31) - 1, -1, N_IMG + 1, N_IMG]
    avg = run_average(c['Y'], c['theta'], c['dx'], order, seg, c['t'])
    ref_avg, ref_cnt = align_ref.class_averages(c['ref'], order, seg)
    assert ref_cnt.tolist() == [294, 0, 0, 59, 38]
    assert (np.abs(avg - ref_avg) <= average_bounds(c['ref'], c['bounds'], order, seg)).all()
    assert not avg[1].any() and not avg[2].any()                         # its only member skipped: an empty class


def test_hostile_seg_is_clamped_on_the_device():
    """seg is replaced by min(max(0, seg[0..k]), N): nothing is followed out of bounds, the result is that of the cleaned seg."""
    n, C = 16, 1
    c = case(n, C)
    seg = np.array([-7, 120, 100, -5, 390, N_IMG + 1000])
    clean = np.array([0, 120, 120, 120, 390, N_IMG])
    avg = run_average(c['Y'], c['theta'], c['dx'], c['order'], seg, c['t'])
    assert np.array_equal(avg, run_average(c['Y'], c['theta'], c['dx'], c['order'], clean, c['t']))
    ref_avg, _ = align_ref.class_averages(c['ref'], c['order'], clean)
    assert (np.abs(avg - ref_avg) <= average_bounds(c['ref'], c['bounds'], c['order'], clean)).all()


def test_unsupported_arguments_are_rejected_and_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    Y = torch.zeros(4, 1, 8, 8, device=DEV)
    th, dx = torch.zeros(4, device=DEV), torch.zeros(4, 2, device=DEV)
    out = torch.full((4, 1, 8, 8), SENT_F, device=DEV)
    order = torch.arange(4, dtype=torch.int32, device=DEV)
    seg = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    avg = torch.full((2, 1, 8, 8), SENT_F, device=DEV)
    wsf = CL.query('tvae_class_average_ws_floats', 4, 2, 1, 8)
    ws = torch.full((wsf,), SENT_F, device=DEV)
    for N, C, n in [(0, 1, 8), (4, 0, 8), (4, 1, 1), (4, 1, 1025), (-4, 1, 8)]:
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():                               # a rejected call must leave every tensor as it was
                CL.call('tvae_align_stack', Y, th, dx, out, N, C, n, 1.0)
    for N, C, n, K, w in [(4, 1, 8, 0, wsf), (4, 1, 8, 65536, wsf), (4, 1, 1, 2, wsf), (0, 1, 8, 2, wsf), (4, 1, 8, 2, wsf - 1)]:
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():
                CL.call('tvae_class_average', Y, th, dx, order, seg, avg, ws, w, N, C, n, K, 1.0)
    assert (out == SENT_F).all() and (avg == SENT_F).all() and (ws == SENT_F).all()


# ---- reproducibility and independence ----------------------------------------------------------------------------------------
def test_python_api_is_bitwise_the_c_abi_and_reproducible():
    from tvae import align
    c = case(33, 3)
    Y, th, dx = _dev(c['Y']), _dev(c['theta']).view(-1, 1), _dev(c['dx'])
    with guardband.GuardedCalls(replay=True):
        a1 = align.align_stack(Y, th, dx, c['t'])
        avg1, cnt1 = align.class_averages(Y, th, dx, c['labels'].copy(), K_CLS, c['t'])
        avg2, cnt2 = align.class_averages(Y, th, dx, torch.from_numpy(c['labels'].copy()).to(DEV), None, c['t'])
    assert np.array_equal(a1.cpu().numpy(), c['got']) and np.array_equal(avg1.cpu().numpy(), c['got_avg'])
    assert torch.equal(avg1, avg2) and cnt1.tolist() == cnt2.tolist() == c['counts'].tolist()
    assert avg1.shape == (K_CLS, 3, 33, 33) and cnt1.dtype == torch.int32 and cnt1.device == Y.device


def test_a_class_does_not_depend_on_the_others():
    c = case(16, 3)
    rng = np.random.default_rng(5)
    labels = c['labels']
    base = c['got_avg']
    # the members of every class but 0 dealt out anew among the classes 1 .. 4 (other sizes, other positions in `order`)
    other = np.flatnonzero(labels != 0)
    shuffled = labels.copy()
    shuffled[other] = rng.integers(1, K_CLS, other.size)
    assert not np.array_equal(shuffled, labels)
    order, seg, _ = align_ref.segments(shuffled, K_CLS)
    assert np.array_equal(run_average(c['Y'], c['theta'], c['dx'], order, seg, c['t'])[0], base[0])
    # and the members of class 0 moved: class 3, whose position in `order` changes, stays bit for bit
    moved = labels.copy()
    moved[np.flatnonzero(labels == 0)[:77]] = 4
    order, seg, _ = align_ref.segments(moved, K_CLS)
    assert np.array_equal(run_average(c['Y'], c['theta'], c['dx'], order, seg, c['t'])[3], base[3])
    # more classes appended: K changes, the first five averages do not
    order, seg, _ = align_ref.segments(labels, K_CLS + 3)
    more = run_average(c['Y'], c['theta'], c['dx'], order, seg, c['t'])
    assert np.array_equal(more[:K_CLS], base) and not more[K_CLS:].any()
    # two labels swapped: the two averages swap
    swapped = np.where(labels == 0, 3, np.where(labels == 3, 0, labels))
    order, seg, _ = align_ref.segments(swapped, K_CLS)
    sw = run_average(c['Y'], c['theta'], c['dx'], order, seg, c['t'])
    assert np.array_equal(sw[0], base[3]) and np.array_equal(sw[3], base[0]) and np.array_equal(sw[[1, 2, 4]], base[[1, 2, 4]])


def test_argument_checks():
    from tvae import align
    from tvae._lib import TvaeHipError
    Y, th, dx = torch.zeros(4, 1, 8, 8, device=DEV), torch.zeros(4, device=DEV), torch.zeros(4, 2, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64)
    for bad in [(Y.double(), th, dx), (Y[:, :, :, ::2], th, dx), (Y.view(4, 8, 8), th, dx), (Y, th[:3], dx), (Y, th, dx[:, :1]),
                (Y, th.cpu(), dx), (torch.zeros(4, 1, 8, 6, device=DEV), th, dx), (torch.zeros(4, 1, 1, 1, device=DEV), th, dx)]:
        with pytest.raises(TvaeHipError):
            align.align_stack(*bad)
        with pytest.raises(TvaeHipError):
            align.class_averages(*bad, lab, 2)
    with pytest.raises(TvaeHipError):
        align.class_averages(Y, th, dx, lab[:3], 2)
    with pytest.raises(TvaeHipError):
        align.class_averages(Y, th, dx, lab, 0)


# ---- the command lines -------------------------------------------------------------------------------------------------------
def test_clustering_particles_writes_class_averages_and_class_averages_py_reproduces_them(tmp_path):
    """clustering_particles.py on tests/golden/stack_ref.mrcs (5 images cropped to 6 x 6, MLP encoder, t = 0.1): with
    TVAE_CLASS_AVERAGES=1 it adds the class-average files, unset the directory is what it was."""
    import src.models as M
    from src import mrc
    from tvae import align
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
        env.pop('TVAE_CLASS_AVERAGES', None)
        env.pop('TVAE_FIGURES', None)
        if mode == 'on':
            env['TVAE_CLASS_AVERAGES'] = '1'
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert ('class averages' in r.stderr) == (mode == 'on')
        listing[mode] = sorted(os.listdir(tmp_path / mode))
    today = ['clusters.npy', 'latents.npy', 'results.txt', 'rotations.npy', 'translations.npy']
    assert listing['off'] == today
    extra = sorted(set(listing['on']) - set(today))
    assert extra in (['class_averages.jpg', 'class_averages.mrcs', 'class_averages.npy', 'class_counts.npy'],
                     ['class_averages.mrcs', 'class_averages.npy', 'class_counts.npy'])
    on = tmp_path / 'on'
    for f in today[:2] + today[3:]:
        assert np.array_equal(np.load(on / f), np.load(tmp_path / 'off' / f)), f
    clusters = np.load(on / 'clusters.npy')
    avg, counts = np.load(on / 'class_averages.npy'), np.load(on / 'class_counts.npy')
    assert avg.shape == (2, 1, 6, 6) and avg.dtype == np.float32
    assert counts.tolist() == np.bincount(clusters, minlength=2).tolist() and counts.sum() == 5
    assert np.array_equal(np.asarray(mrc.open_stack(str(on / 'class_averages.mrcs'))[0]), avg.reshape(2, 6, 6))
    # bitwise tvae.align.class_averages of the saved pose and label files
    Y = torch.from_numpy(align.load_stack(stack, 6)).to(DEV)
    th = torch.from_numpy(np.load(on / 'rotations.npy').astype(np.float32)).to(DEV)
    dx = torch.from_numpy(np.load(on / 'translations.npy').astype(np.float32)).to(DEV)
    want, wcnt = align.class_averages(Y, th, dx, clusters, 2, align.translation_scale('unimodal'))
    assert np.array_equal(want.cpu().numpy(), avg) and wcnt.tolist() == counts.tolist()
    Yh, dxh = Y.cpu().numpy(), dx.cpu().numpy()
    ref = align_ref.align_stack(Yh, th.cpu().numpy(), dxh, float(np.float32(0.1)))
    order, seg, _ = align_ref.segments(clusters, 2)
    ref_avg, _ = align_ref.class_averages(ref, order, seg)
    assert (np.abs(avg - ref_avg) <= average_bounds(ref, image_bounds(Yh, dxh, 0.1), order, seg)).all()
    # class_averages.py: the same from the files alone
    cmd = [sys.executable, os.path.join(PKG, 'class_averages.py'), '--stack', stack, '--crop', '6', '--t-inf', 'unimodal',
           '--rotations', str(on / 'rotations.npy'), '--translations', str(on / 'translations.npy'),
           '--clusters', str(on / 'clusters.npy'), '--out-dir', str(tmp_path / 'again'), '--write-aligned']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    again = tmp_path / 'again'
    assert np.array_equal(np.load(again / 'class_averages.npy'), avg) and np.array_equal(np.load(again / 'class_counts.npy'), counts)
    assert open(again / 'class_averages.mrcs', 'rb').read() == open(on / 'class_averages.mrcs', 'rb').read()
    aligned = np.load(again / 'aligned.npy')
    assert aligned.shape == (5, 1, 6, 6) and np.array_equal(aligned, align.align_stack(Y, th, dx, 0.1).cpu().numpy())
