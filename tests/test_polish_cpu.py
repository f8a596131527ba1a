"""Sub-pixel pose polish, the part that needs no GPU: the fp64 restatement tests/polish_ref.py itself -- its template and sums
against tests/pose_ref.py, its derivatives against central differences, convergence on planted poses, monotone scores and the
trust region with and without noise, the images it must leave alone -- and the parser of polish_poses.py."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import polish_ref
import pose_ref
from conftest import PKG

F32 = np.float32
I = polish_ref.IDX


def _hostile_inputs(n=8, C=2, seed=4):
    """12 images in K = 3 classes: generic poses, two labels outside [0, K), four hostile poses, one fully out of frame."""
    rng = np.random.default_rng(seed)
    N, K = 12, 3
    refs = rng.standard_normal((K, C, n, n)).astype(F32)
    Y = rng.standard_normal((N, C, n, n)).astype(F32)
    theta = rng.uniform(-np.pi, np.pi, N).astype(F32)
    dx = rng.uniform(-0.3, 0.3, (N, 2)).astype(F32)
    cls = rng.integers(0, K, N)
    cls[2], cls[3] = -1, 7
    theta[4] = np.nan
    dx[5], dx[6], dx[7], dx[8] = (1e30, 0.0), (0.0, np.inf), (np.nan, 0.1), (3.0, 0.0)
    return Y, refs, theta, dx, cls, [2, 3], [4, 5, 6, 7, 8]


# ---- 1. the shared sums -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True])
def test_template_and_shared_sums_are_those_of_pose_ref(masked):
    Y, refs, theta, dx, cls, skipped, hostile = _hostile_inputs()
    for t in (1.0, 0.1):
        radius, edge = (2.5, 2.0) if masked else (None, 0.0)
        d = (dx / F32(t)).astype(F32)
        b = polish_ref.basis(refs, cls, theta, d, t, radius, edge)
        mom = polish_ref.moments(Y, b)
        T = pose_ref.templates(refs, cls, theta, d, t, 0, 0.0, 0, radius, edge)
        num, pp, yy = pose_ref.tables(Y, T, 0)
        assert np.array_equal(b['P'], T[:, 0])
        # the same products; numpy's pairwise sums run over differently laid out arrays: equal to a few fp64 roundings
        near = lambda a, c, scale: (np.abs(a - c) <= 64 * 2.0 ** -53 * scale).all()
        aP, aY = np.abs(T[:, 0]), np.abs(Y.astype(np.float64))
        assert near(mom[:, I['PP']], pp[:, 0, 0, 0], pp[:, 0, 0, 0])
        assert near(mom[:, I['PY']], num[:, 0, 0, 0], (aP * aY).sum(axis=(1, 2, 3)))
        live = np.setdiff1d(np.arange(cls.size), skipped)
        assert near(mom[live, I['YY']], yy[live], yy[live])
        assert not mom[skipped].any()                                    # 15 zeros
        assert not mom[hostile, :14].any() and (mom[hostile, 14] > 0).all()      # zeros and the true yy
        assert np.isfinite(mom).all()
        generic = np.setdiff1d(live, hostile)
        assert (mom[generic, I['DD']] > 0).all() and (mom[generic, I['G0G0']] > 0).all()


# ---- 2. the derivatives -----------------------------------------------------------------------------------------------------------
def test_derivatives_agree_with_central_differences_of_the_templates():
    """Step 1e-4 px for the translations and 419 * 2^-22 = 0.99897e-4 rad for the angle (angles are multiples of 2^-6, so that
    theta +- h are fp32 numbers and pose_ref.templates, which takes the angle in fp32, sees exactly them).  Only samples whose
    cell is the same at both ends and in the middle count.  Within a cell the sample is bilinear, B(p + d) = B(p) + g . d +
    X dc dr with X the cell's mixed second difference.
      translation: the position moves along a straight line, the quadratic term is even and cancels: the central difference
        is exact, and the tolerance is the fp64 rounding of the two templates (positions off by at most 20 n 2^-53 px, a
        value by 8 * 2^-53 max |ref|), divided by 2 h;
      angle: the position moves by +-o + e with |o| <= R h and |e| <= R h^2 / 2 (R the distance of u from the centre in
        pixels): the central difference is Dtheta sin(h) / h + X (oc er + or ec) / h, so the second-order term is at most
        |Dtheta| h^2 / 6 + Xmax R^2 h^2, with Xmax the largest mixed second difference of the zero-bordered references."""
    for n, t in ((32, 1.0), (33, 0.1)):
        K, N = 3, 10
        rng = np.random.default_rng(n)
        refs = pose_ref.smooth_refs(n, K, C=2, seed=n)
        cls = rng.integers(0, K, N)
        theta = (rng.integers(-192, 193, N) / 64.0).astype(F32)
        dx = (rng.uniform(-0.2, 0.2, (N, 2)) / t).astype(F32)
        b = polish_ref.basis(refs, cls, theta, dx, t)
        Dtx, Dty = polish_ref.translation_basis(b, theta)
        pad = np.pad(refs.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
        gmax = max(np.abs(np.diff(pad, axis=2)).max(), np.abs(np.diff(pad, axis=3)).max())
        xmax = np.abs(np.diff(np.diff(pad, axis=2), axis=3)).max()
        round_tol = (20 * n * 2.0 ** -53 * gmax + 8 * 2.0 ** -53 * np.abs(refs).max())
        half = (n - 1) / 2

        def cells(th, d):
            p = polish_ref.positions(n, th, d, t)
            return np.floor(p['col']), np.floor(p['row']), p['inside']

        def same_cell(plus, minus):
            c0, r0, in0 = cells(theta, dx)
            ok = in0
            for th, d in (plus, minus):
                c, r, i = cells_f64(th, d)
                ok = ok & i & (c == c0) & (r == r0)
            assert ok.sum() > 0.99 * in0.sum() > 0.7 * in0.size           # (nearly every sample inside the frame is checked)
            return ok

        def cells_f64(th, d):
            col, row, _ = pose_ref.template_positions(n, 0, th, d, t)
            return np.floor(col), np.floor(row), (col > -1) & (col < n) & (row > -1) & (row < n)

        # translations: h pixels = h / half coordinate units = h / half / t of dx
        h = 1e-4
        for axis, want in ((0, Dtx), (1, Dty)):
            e = np.zeros(2)
            e[axis] = h / half / float(F32(t))
            dp, dm = dx.astype(np.float64) + e, dx.astype(np.float64) - e
            Tp = pose_ref.templates(refs, cls, theta, dp, t, 0, 0.0, 0)[:, 0]
            Tm = pose_ref.templates(refs, cls, theta, dm, t, 0, 0.0, 0)[:, 0]
            cd = (Tp - Tm) / (2 * h / half)                              # per coordinate unit, as Dtx and Dty are
            ok = same_cell((theta, dp), (theta, dm))
            err = np.abs(cd - want)[np.broadcast_to(ok[:, None], cd.shape)]
            tol = round_tol / (2 * h / half)
            print(f'polish_ref n={n} axis {axis}: central difference off by {err.max():.3e}, tolerance {tol:.3e}')
            assert err.max() <= tol
        # the angle
        ha = 419 * 2.0 ** -22
        thp, thm = (theta + F32(ha)).astype(F32), (theta - F32(ha)).astype(F32)
        assert np.array_equal(thp.astype(np.float64), theta.astype(np.float64) + ha)
        assert np.array_equal(thm.astype(np.float64), theta.astype(np.float64) - ha)
        Tp = pose_ref.templates(refs, cls, thp, dx, t, 0, 0.0, 0)[:, 0]
        Tm = pose_ref.templates(refs, cls, thm, dx, t, 0, 0.0, 0)[:, 0]
        cd = (Tp - Tm) / (2 * ha)
        ok = same_cell((thp, dx), (thm, dx))
        R = b['pos']['d'][:, None]
        tol = np.abs(b['D']) * ha * ha / 6 + xmax * R * R * ha * ha + round_tol * (1 + R) / (2 * ha)
        okb = np.broadcast_to(ok[:, None], cd.shape)
        err = np.abs(cd - b['D'])
        print(f'polish_ref n={n} angle: central difference off by {err[okb].max():.3e}, worst error / tolerance '
              f'{(err[okb] / tol[okb]).max():.3f}')
        assert (err[okb] <= tol[okb]).all()
        assert np.abs(b['D'][okb]).max() > 1.0                           # (the tolerance is small against what it bounds)


# ---- 3. convergence, monotonicity, the trust region ---------------------------------------------------------------------------------
MAX_SHIFT, MAX_ANGLE, ITERATIONS = 1.0, 0.05, 8


@functools.lru_cache(maxsize=None)
def off_grid_case(n, sigma=0.0, masked=False, t=1.0):
    """pose_ref.planted(n, N = 48) with starts off the grid by U(-0.7, 0.7) px per axis and U(-0.04, 0.04) rad, noise of
    standard deviation sigma on the images, polished by the fp64 restatement."""
    p = pose_ref.planted(n=n, N=48, t=t)
    rng = np.random.default_rng(1000 + n)
    th0 = (p['theta_true'] + rng.uniform(-0.04, 0.04, 48)).astype(F32)
    dx0 = (p['dx_true'] + rng.uniform(-0.7, 0.7, (48, 2)) * 2 / (n - 1) / t).astype(F32)
    Y = p['Y'] if sigma == 0 else (p['Y'] + sigma * rng.standard_normal(p['Y'].shape)).astype(F32)
    radius, edge = (0.4 * n, 3.0) if masked else (None, 0.0)
    r = polish_ref.polish(Y, th0, dx0, p['cls'], p['refs'], t, ITERATIONS, MAX_SHIFT, MAX_ANGLE, radius, edge)
    return p, Y, th0, dx0, r


def _errors(p, theta, dx, n, t=1.0):
    """(shift error in pixels, angle error in radians) per image against the planted poses."""
    es = np.abs(np.asarray(dx, dtype=np.float64) - p['dx_true']).max(1) * t * (n - 1) / 2
    ea = np.abs(np.asarray(theta, dtype=np.float64) - p['theta_true'])
    return es, ea


@pytest.mark.parametrize('n', [32, 33, 64])
def test_planted_poses_are_recovered_without_noise(n):
    p, Y, th0, dx0, r = off_grid_case(n)
    s0, a0 = _errors(p, th0, dx0, n)
    s1, a1 = _errors(p, r['theta'], r['dx'], n)
    print(f'polish_ref n={n}: shift error {s0.max():.3f} -> {s1.max():.3e} px, angle error {a0.max():.3f} -> {a1.max():.3e} rad, '
          f'accepted steps {r["steps"].min()} .. {r["steps"].max()}, mean score {r["score"][:, 0].mean():.6f} -> '
          f'{r["score"][:, 1].mean():.6f}')
    assert s0.max() > 0.5 and a0.max() > 0.03                            # (the starts are really off)
    assert s1.max() <= 1e-6 and a1.max() <= 1e-6
    assert (r['score'][:, 1] > 1 - 1e-6).all()


@pytest.mark.parametrize('n,sigma,masked,t', [(32, 0.0, False, 1.0), (33, 0.0, False, 1.0), (64, 0.0, False, 1.0),
                                               (32, 0.3, False, 1.0), (64, 1.0, False, 1.0), (32, 0.0, True, 1.0),
                                               (32, 1.0, True, 0.1), (33, 0.3, False, 0.1)])
def test_scores_never_fall_and_no_pose_leaves_the_trust_region(n, sigma, masked, t):
    p, Y, th0, dx0, r = off_grid_case(n, sigma, masked, t)
    assert (r['score'][:, 1] >= r['score'][:, 0]).all() and np.isfinite(r['score']).all()
    ra, rd, _ = polish_ref.radii(n, t, MAX_SHIFT, MAX_ANGLE)
    assert abs(rd - MAX_SHIFT * 2 / (n - 1) / float(F32(t))) <= 1e-15 * rd and ra == float(F32(MAX_ANGLE))
    assert (np.abs(r['theta'].astype(np.float64) - th0) <= ra).all()
    assert (np.abs(r['dx'].astype(np.float64) - dx0) <= rd).all()
    assert (r['steps'] >= 0).all() and (r['steps'] <= ITERATIONS).all()
    s0, _ = _errors(p, th0, dx0, n, t)
    s1, _ = _errors(p, r['theta'], r['dx'], n, t)
    print(f'polish_ref n={n} sigma={sigma} mask={masked} t={t}: median shift error {np.median(s0):.3f} -> {np.median(s1):.3f} px, '
          f'largest {s0.max():.3f} -> {s1.max():.3f}')
    if masked and sigma == 0:
        assert s1.max() <= 0.01                                          # the optimum itself moves by about 1e-3 px under the mask


def test_a_tight_trust_region_is_reached_and_kept():
    p, Y, th0, dx0, _ = off_grid_case(32)
    r = polish_ref.polish(Y, th0, dx0, p['cls'], p['refs'], 1.0, ITERATIONS, 0.25, 0.01)
    ra, rd, _ = polish_ref.radii(32, 1.0, 0.25, 0.01)
    da, dd = np.abs(r['theta'].astype(np.float64) - th0), np.abs(r['dx'].astype(np.float64) - dx0)
    assert (da <= ra).all() and (dd <= rd).all()
    assert (dd.max(1) > 0.99 * rd).sum() > 10                            # many starts are further off than the region allows
    assert (r['score'][:, 1] >= r['score'][:, 0]).all()
    zero = polish_ref.polish(Y, th0, dx0, p['cls'], p['refs'], 1.0, 3, 0.0, 0.0)
    assert np.array_equal(zero['theta'].view(np.int32), th0.view(np.int32))
    assert np.array_equal(zero['dx'].view(np.int32), dx0.view(np.int32)) and not zero['steps'].any()


# ---- 4. the images that must be left alone --------------------------------------------------------------------------------------
def test_skipped_and_hostile_images_keep_their_pose_bit_for_bit():
    Y, refs, theta, dx, cls, skipped, hostile = _hostile_inputs()
    r = polish_ref.polish(Y, theta, dx, cls, refs, 1.0, 4, 1.0, 0.05)
    alone = skipped + hostile
    assert np.array_equal(r['theta'][alone].view(np.int32), theta[alone].view(np.int32))
    assert np.array_equal(r['dx'][alone].view(np.int32), dx[alone].view(np.int32))
    assert not r['score'][alone].any() and not r['steps'][alone].any()
    rest = np.setdiff1d(np.arange(cls.size), alone)
    assert r['steps'][rest].sum() > 0 and (r['score'][rest, 1] >= r['score'][rest, 0]).all()
    # nothing of a reference is read for a skipped image, and the empty class may hold anything
    nan = polish_ref.polish(Y, theta, dx, np.where(np.isin(np.arange(cls.size), rest), -1, cls), np.full_like(refs, np.nan), 1.0, 2)
    assert np.array_equal(nan['theta'].view(np.int32), theta.view(np.int32)) and not nan['score'].any()


def test_the_step_on_degenerate_moments_is_no_step():
    """Zero or non-finite pivots, PP = 0 and YY = 0 mean "no step": the trial is the current pose and the image ends."""
    cur = (F32(0.3), F32(0.1), F32(-0.2))
    good = np.array([4.0, 0.1, 0.2, -0.1, 9.0, 0.5, -0.4, 7.0, 0.3, 6.0, 3.0, 0.7, -0.6, 0.5, 5.0])
    tr, exact = polish_ref.trial(good, cur, cur, 1e-3, 32, 1.0, 1.0, 0.05)
    assert exact is not None and not polish_ref.same_bits(tr, cur)
    for k, v in (('PP', 0.0), ('YY', 0.0), ('DD', np.nan), ('G0G0', np.inf)):
        m = good.copy()
        m[I[k]] = v
        tr, exact = polish_ref.trial(m, cur, cur, 1e-3, 32, 1.0, 1.0, 0.05)
        assert exact is None and polish_ref.same_bits(tr, cur), k
    m = np.zeros(15)
    m[[I['PP'], I['PY'], I['YY']]] = 1.0                                 # no derivative at all: every pivot but the last is 0
    assert polish_ref.trial(m, cur, cur, 1e-3, 32, 1.0, 1.0, 0.05)[1] is None
    assert polish_ref.score(m) == 1.0 and polish_ref.score(np.zeros(15)) == 0.0


# ---- 5. the parser ------------------------------------------------------------------------------------------------------------------
def _flags(p):
    return sorted(s for a in p._actions for s in a.option_strings if a.dest != 'help')


def test_parser_of_polish_poses_py():
    from tvae import refine
    before = _flags(refine.build_parser())
    from tvae import polish
    p = polish.build_parser()
    assert _flags(p) == sorted(['--stack', '--rotations', '--translations', '--clusters', '--t-inf', '--crop', '--n-clusters',
                                '--out-dir', '-d', '--device', '--rounds', '--mask-radius', '--mask-edge', '--cross-halves',
                                '--iterations', '--max-shift', '--max-angle'])
    need = ['--stack', 's.npy', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy']
    a = p.parse_args(need)
    assert (a.rounds, a.iterations, a.max_shift, a.mask_radius, a.mask_edge, a.cross_halves) == (1, 8, 1.0, None, 0.0, False)
    assert abs(np.radians(a.max_angle) - 0.05) < 1e-12 and (a.t_inf, a.crop, a.device, a.n_clusters) == ('attention', 0, 0, None)
    a = p.parse_args(need + ['--iterations', '3', '--max-shift', '0.5', '--max-angle', '1.5', '--cross-halves', '--rounds', '2'])
    assert (a.iterations, a.max_shift, a.max_angle, a.cross_halves, a.rounds) == (3, 0.5, 1.5, True, 2)
    with pytest.raises(SystemExit):
        p.parse_args(need + ['--shift', '2'])                            # the grid search's flags are not the polish's
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's.npy'])
    # the parser it borrows from is what it was
    after = refine.build_parser()
    assert _flags(after) == before == sorted(['--stack', '--rotations', '--translations', '--clusters', '--t-inf', '--crop',
                                              '--n-clusters', '--out-dir', '-d', '--device', '--rounds', '--angle-range',
                                              '--angle-steps', '--shift', '--mask-radius', '--mask-edge', '--cross-halves'])
    assert after.parse_args(need).rounds == 3
    spec = importlib.util.spec_from_file_location('polish_poses_script', os.path.join(PKG, 'polish_poses.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run is polish.run and callable(mod.main)


def test_the_binding_declares_the_two_entry_points_as_the_header_does():
    from tvae import _cluster_lib, _lib
    assert _cluster_lib.SIGNATURES['tvae_pose_moments'] == 'pppppp' + 'iiii' + 'fff'
    assert _cluster_lib.SIGNATURES['tvae_pose_polish_step'] == 'p' * 13 + 'iiii' + 'fff'
    assert ('tvae_pose_polish_step', 10) in _lib._F64_OK and _cluster_lib.ABI_VERSION == 1
