"""The CTF in the template without a GPU: the host side (parser, bindings, header) and the fp64 restatement
tests/ctf_pose_ref.py against identities it must satisfy -- Parseval, the adjoint identity that lets the middle term of the
residual come from the filtered stack, the independence of the last term from the shift -- the fp32 emulation of the two DFT
stages inside the a-priori bound on every case of test_ctf_pose_gpu.py, and the planted stack on which the CTF round beats the
plain one."""
import inspect
import os
import re

import numpy as np
import pytest

import align_ref
import ctf_pose_ref as R
import ctf_ref
import ml_ref
import pose_ref
from conftest import ROOT


# ---- the host side -----------------------------------------------------------------------------------------------------------------
def test_parser_with_ctf_adds_its_flags_and_the_default_is_unchanged():
    from tvae import ml2d
    plain = {a.dest for a in ml2d.build_parser()._actions}
    assert plain == {a.dest for a in ml2d.build_parser(ctf=False)._actions}
    with_ctf = {a.dest: a for a in ml2d.build_parser(ctf=True)._actions}
    assert set(with_ctf) - plain == {'ctf', 'wiener_tau', 'scale'}
    assert with_ctf['ctf'].default is None and with_ctf['wiener_tau'].default == 0.1 and with_ctf['scale'].default == 1
    assert 'ctf_correct' not in with_ctf
    args = ml2d.build_parser(ctf=True).parse_args(['--stack', 's', '--rotations', 'r', '--translations', 't', '--clusters', 'c',
                                                   '--ctf', 'ctf.txt', '--wiener-tau', '0.25'])
    assert args.ctf == 'ctf.txt' and args.wiener_tau == 0.25


def test_public_functions_and_their_arguments():
    from tvae import ctf, ml2d
    sig = inspect.signature(ml2d.ml_rounds).parameters
    assert sig['ctf'].default is None and sig['wiener_tau'].default == 0.1
    assert list(sig)[-2:] == ['ctf', 'wiener_tau']            # behind every argument that existed: positional calls stand
    assert list(inspect.signature(ctf.template_power).parameters) == ['theta', 'dx', 'slots', 'refs', 'coef', 't_scale',
                                                                      'angle_steps', 'angle_step', 'mask_radius', 'mask_edge']
    assert list(inspect.signature(ctf.power_weighted).parameters) == ['coef', 'entries', 'n', 'n_clusters']


def test_header_and_binding_declare_the_entry_points():
    from tvae import _cluster_lib as CL
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
    for name in ('tvae_template_ctf_power', 'tvae_ctf_power_entries'):
        assert name in CL.SIGNATURES and re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
    assert CL.QUERIES['tvae_template_ctf_power_ws_floats'] == ('iiiii', 'l')
    assert re.search(r'\blong\s+tvae_template_ctf_power_ws_floats\s*\(', hdr)
    assert CL.ABI_VERSION == 1                                # nothing that existed changed
    L = CL.lib()
    q = lambda *a: CL.query('tvae_template_ctf_power_ws_floats', *a)
    assert q(5, 1, 64, 4, 8) == 2 and q(1 << 24, 16, 128, 1, 0) == 2
    for bad in [(0, 1, 64, 4, 8), (5, 17, 64, 4, 8), (5, 1, 1, 4, 8), (5, 1, 129, 4, 8), (5, 1, 64, 0, 8), (5, 1, 64, 65, 8),
                (5, 1, 64, 4, -1), (5, 1, 64, 4, 33), (1 << 24, 1, 64, 64, 32)]:          # (the last: N M NA >= 2^31)
        assert q(*bad) == 0, bad
    assert hasattr(L, 'tvae_ctf_power_entries')


# ---- identities of the restatement ---------------------------------------------------------------------------------------------------
def _small(n, C=1, M=2, A=1, masked=False, seed=0):
    rng = np.random.default_rng([n, seed])
    refs = pose_ref.smooth_refs(n, 3, C, seed=seed + 1)
    N = 4
    theta = rng.uniform(-np.pi, np.pi, N).astype(np.float32)
    dx = rng.uniform(-0.1, 0.1, (N, 2)).astype(np.float32)
    cand = rng.integers(0, 3, (N, M))
    mask = (0.3 * n, 0.15 * n) if masked else (None, 0.0)
    return refs, cand, theta, dx, mask


@pytest.mark.parametrize('n,C,masked', [(9, 1, False), (16, 2, True), (33, 1, True)])
def test_parseval(n, C, masked):
    """coef = (0, 1, 0, 0, 0) is H = 1 everywhere: ppc is the sum of T^2."""
    refs, cand, theta, dx, mask = _small(n, C, masked=masked)
    coef = np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (4, 1))
    assert np.array_equal(ctf_ref.H(coef, n), np.ones((4, n, n // 2 + 1)))
    ppc, T = R.template_power(refs, cand, theta, dx, coef, 1.0, 1, 0.05, *mask)
    want = (T ** 2).sum((-3, -2, -1))
    assert want.min() > 0 and (np.abs(ppc - want) <= 1e-13 * want).all()


@pytest.mark.parametrize('n', [9, 16, 33])
def test_adjoint_identity(n):
    """<Y, H (*) P> = <H (*) Y, P> to fp64 rounding: H is real and even, so the circular filter is self-adjoint, and the middle
    term of the residual is the num table of the filtered stack."""
    rng = np.random.default_rng(n)
    Y, P = rng.standard_normal((5, 1, n, n)), rng.standard_normal((5, 1, n, n))
    coef = R.defocus_rows(n, 5)
    a = (Y * R.filtered(P, coef)).sum((1, 2, 3))
    b = (R.filtered(Y, coef) * P).sum((1, 2, 3))
    scale = np.sqrt((Y ** 2).sum((1, 2, 3)) * (P ** 2).sum((1, 2, 3)))
    assert (np.abs(a - b) <= 1e-13 * scale).all() and (np.abs(a) > 1e-3 * scale).any()
    # and the residual itself, expanded: |Y - H P|^2 = |Y|^2 - 2 <H Y, P> + |H P|^2 with the last term in Fourier space
    r = ((Y - R.filtered(P, coef)) ** 2).sum((1, 2, 3))
    last = R.power_of(P, R.h_full(coef, n))
    assert (np.abs(r - ((Y ** 2).sum((1, 2, 3)) - 2 * b + last)) <= 1e-12 * r).all()


def test_shift_independence():
    """ppc is |H (*) P|^2 of EVERY shifted window of the extended template while the masked support moved by S stays inside the
    frame (the shift is then circular: a phase factor), and differs measurably where the support leaves the frame."""
    n, S = 24, 2
    coef = R.defocus_rows(n, 2, 0.6)[:1]
    g = np.arange(n) - (n - 1) / 2
    jj, ii = np.meshgrid(g, g)
    blob = lambda ci, cj: np.exp(-((ii - ci) ** 2 + (jj - cj) ** 2) / (2 * 2.0 ** 2))[None, None]
    inside, outside = blob(1.0, -2.0).astype(np.float32), blob(1.0, 10.5).astype(np.float32)
    theta, dx, cls = np.array([0.3], dtype=np.float32), np.array([[0.02, -0.03]], dtype=np.float32), np.array([0])
    radius, edge = 6.0, 2.0                                   # the support ends 8 pixels from the centre: 3.5 + S inside the frame
    Hf = R.h_full(coef, n)
    # the mask is centred on the object: the blob at the border is cut by the frame only without it
    for ref, same, mask in ((inside, True, (radius, edge)), (outside, False, (None, 0.0))):
        ppc, _ = R.template_power(ref, cls[:, None], theta, dx, coef, 1.0, 0, 0.0, *mask)
        Te = pose_ref.templates(ref, cls, theta, dx, 1.0, 0, 0.0, S, *mask)[:, 0]                  # [1][C][ne][ne]
        worst = 0.0
        for sy in range(2 * S + 1):
            for sx in range(2 * S + 1):
                win = Te[:, :, sy:sy + n, sx:sx + n]
                worst = max(worst, abs(float(R.power_of(win, Hf)[0]) - float(ppc[0, 0, 0])) / float(ppc[0, 0, 0]))
        if same:
            assert worst <= 1e-12, worst
        else:
            assert worst >= 1e-3, worst


@pytest.mark.parametrize('geometry', R.GPU_CASES)
def test_fp32_emulation_is_inside_the_bound(geometry):
    """Every case of test_ctf_pose_gpu.py, without the kernel: the float32 restatement of the two stages stays inside the
    a-priori bound, the bound is at most 1 % of the reference (the cap: a looser bound would say little), and the slots that
    must be exact zeros are."""
    c = R.gpu_case(*geometry)
    ref, bound = c['ref'], c['bound']
    valid = (c['cand'] >= 0) & (c['cand'] < R.K_CLS)
    assert (ref[valid] > 0).all() and not ref[~valid].any() and not bound[~valid].any()
    f32 = R.template_power_f32(c['T'], c['coef'])
    assert (np.abs(f32 - ref) <= bound).all()
    assert (bound[valid] <= 1e-2 * ref[valid]).all(), (bound[valid] / ref[valid]).max()
    assert (c['coef'][:, 4] >= 0).all()                       # the contract of tvae_ctf_eval is stated for c4 q >= 0


def test_power_weighted_restatement():
    """Unit weights over a partition give ctf_ref.power; dead entries and a broken seg change nothing they should not."""
    n, N, K = 12, 9, 3
    rng = np.random.default_rng(5)
    coef = R.defocus_rows(n, N)
    lab = rng.integers(0, K, N)
    order, seg, _ = align_ref.segments(lab, K)
    D0, c0 = ctf_ref.power(coef, order, seg, n)
    D, W, cnt = R.power_weighted(coef, order, np.ones(N, dtype=np.float32), seg, n)
    assert np.array_equal(D, D0) and cnt.tolist() == c0.tolist() and W.tolist() == c0.astype(float).tolist()
    img = np.concatenate([order, [-1, 2, 3, N]])
    w = np.concatenate([np.ones(N), [1.0, 0.0, np.nan, 1.0]]).astype(np.float32)
    seg2 = np.array(seg)
    seg2[-1] = N + 4
    D2, W2, cnt2 = R.power_weighted(coef, img, w, seg2, n)
    assert np.array_equal(D2, D0) and np.array_equal(W2, W) and cnt2.tolist() == c0.tolist()
    D3, _, cnt3 = R.power_weighted(coef, order, np.ones(N, dtype=np.float32), [5, -3, 99, 2], n)   # cleaned: 5, 5, 9, 9
    assert cnt3.tolist() == [0, 4, 0] and not D3[0].any() and not D3[2].any()


# ---- the planted stack ----------------------------------------------------------------------------------------------------------------
def _distance(avg, refs):
    """|avg_k - ref_k|_2 / |ref_k|_2 per class."""
    d = np.sqrt(((np.asarray(avg, dtype=np.float64) - refs) ** 2).sum((1, 2, 3)))
    return d / np.sqrt((np.asarray(refs, dtype=np.float64) ** 2).sum((1, 2, 3)))


def test_ctf_round_beats_the_plain_round_on_a_planted_stack():
    """pose_ref.planted seen through eight defoci with noise added: the averages of the CTF round are closer to the planted objects
    than those of the plain ml_ref.rounds of the same stack, which averages images whose transfer functions have their zeros and
    signs elsewhere.  The ordering is asserted for every class, not a figure."""
    p = R.loop_case()
    L = R.LOOP
    args = dict(rounds=L['rounds'], angle_range=p['A'] * p['dtheta'], A=p['A'], S=p['S'], keep=L['keep'])
    with_ctf = R.rounds(p['Y'], p['theta'], p['dx'], p['cls'], p['K'], p['coef'], p['t'], tau=L['tau'], **args)
    plain = ml_ref.rounds(p['Y'], p['theta'], p['dx'], p['cls'], p['K'], p['t'], **args)
    d_ctf, d_plain = _distance(with_ctf['avg'], p['refs']), _distance(plain['avg'], p['refs'])
    print(f'distance to the planted objects: CTF round {d_ctf.tolist()}, plain round {d_plain.tolist()}')
    assert (d_plain > 0.3).all()                              # the plain route is visibly wrong
    assert (d_ctf < d_plain).all()
    assert np.isfinite(with_ctf['log_likelihood']).all() and with_ctf['D'].shape == (p['K'], p['n'], p['n'] // 2 + 1)


def test_loop_case_of_the_gpu_test_stays_within_its_caps():
    """What test_ctf_pose_gpu.py's comparison of the loop relies on, checked on the reference alone: at most 5 % of the images
    are left out for a runner-up margin within the tolerance, the top-P sets are clear of it in both rounds, the float32
    restatement of the loop reaches the reference's labels, and its tolerances are small against what they bound."""
    p, ref, tol = R.loop_tolerance()
    _, emu = R.loop_reference(True)
    print(f"loop: dl {tol['dl']:.3e}, |avg| tolerance {tol['avg'].tolist()}, left out {int(tol['left_out'].sum())} of {p['N']}")
    assert tol['left_out'].mean() <= 0.05
    assert tol['cut_clear']
    assert np.array_equal(emu['labels'], ref['labels'])
    assert np.array_equal(np.sort(emu['post']['idx'], 1), np.sort(ref['post']['idx'], 1))
    assert (tol['avg'] <= 1e-4 * np.sqrt((ref['avg'] ** 2).sum((1, 2, 3)))).all() and tol['dl'] < 1e-2
    assert ref['post']['live'].all() and len(set(ref['labels'].tolist())) == p['K']
