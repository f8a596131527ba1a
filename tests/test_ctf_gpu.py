"""CTF correction on the GPU: tvae_ctf_eval, tvae_fourier_filter and tvae_ctf_power behind their C ABI (every call under
guard bands with replay, outputs and workspace filled with a sentinel) against the fp64 restatement tests/ctf_ref.py, then
tvae.ctf (filter_bank against the reference's own filters, the two CTF-corrected class averages, the recovery of a known
image) and the --ctf flags of class_averages.py and class_resolution.py.

u = 2^-24.  H: the contract of the header, |H_gpu - H_fp64| <= 8 u (|c0| + |c1|).

Filter, tolerance (a): a Frobenius bound per plane, a priori.  An fp32 FMA chain of L products errs by at most
g_L sum |a_k| |b_k| with g_L = (L + 2) u (L u for the chain, one u for the rounding of a twiddle, one of slack), and by
Cauchy-Schwarz sum |a_k| |b_k| <= |a|_2 |b|_2; the twiddles have unit modulus, so cos^2 + sin^2 sums to the length.
    stage 1 (real rows, L = n):      |E1(i, kx)| <= g_n sqrt(n) |x_i|_2                (re and im together)
    stages 2, 3 (complex, L = 2 n):  |E(a, kx)|  <= sqrt(2) g_2n sqrt(n) |v_kx|_2      (v_kx the input column)
    multiply:                        u |F'| for the rounding and, with coefficients, 8 u (|c0| + |c1|) w |F| for H itself
    stage 4 (real output, L = 2 R):  |E4(i, j)|  <= g_2R sqrt(R) |P_i|_2 / n^2
    store:                           u |ref|
An error in the spectrum F' (weights included) reaches the output through Re of a matrix with orthogonal columns of norm n,
divided by n^2: a factor 1 / n in Frobenius norm; a column DFT multiplies a column's norm by sqrt(n), the row stage back
by at most sqrt(n).  With F' = H w F, hw = |H| w and |.| Frobenius norms of the fp64 reference's own arrays:
    bound = g_n |x| sqrt(sum_kx max_ky hw^2) + sqrt(2) g_2n n^-1/2 sqrt(sum_kx |G_kx|^2 sum_ky hw^2)
            + (u |F'| + 8 u c01 |w F|) / n + sqrt(2) g_2n n^-1/2 |F'| + g_2R sqrt(R) |F'| / n + u |ref|
(tests/ctf_ref.py: filter_bound).  Every case is seeded until bound <= 1e-2 |ref_b|_2 in every plane.
Tolerance (b), per element: 8 x the largest per-element error, over the planes of the case, of the float32 numpy restatement
of the same four stages (ctf_ref.filter_f32) against fp64, computed here on the CPU; the 8 covers the different summation
order (a sequential FMA chain against numpy's blocked sums).

Power: |D - ref| <= 2 * 8 u (|c0| + |c1|) sum |H_i| (the contract, through the square) + (m + 2) 2^-52 sum H_i^2 (the fp64
sum of the m members).

Class averages (test 7), relative Frobenius error per class.  x'_i = filter(x_i) errs by at most a_i = bound (a); the
bilinear alignment is a matrix with row sums <= 1 and column sums <= c_i, so of norm <= sqrt(c_i) (c_i computed from the
reference's own sampling positions); the aligned mean adds the per-element bound of test_align_gpu.py (average_bounds), in
Frobenius norm.  flip: that is all.  wiener: G = 1 / (D / m + tau) <= 1 / tau, its relative error is u (the one rounding)
plus G dD / m <= 16 u c01 max |H| / tau; the last filter multiplies an incoming error by at most max G and adds its own
bound (a) with the plane G:
    tol_k = max G_k ((1 / m) sum_i sqrt(c_i) a_i + |average_bounds_k|) + rel_G max G_k |mean_k| + a(mean_k, G_k).
The test asserts tol_k <= 1e-3 |ref_k|.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref
import ctf_ref
import guardband
from conftest import PKG, load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 2.0 ** -24
SENT_F = -12345.5
B_IMG = 5
SIZES = (2, 3, 8, 31, 33, 64, 65, 96, 127, 128, 129)        # 128 | 129: the spectrum in LDS | through the workspace


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV, dtype).contiguous()


def table(rng, N, bfactor=(50.0, 150.0), ampcont=7.0):
    """N realistic rows of the eight-column table: defocus 1-3 um, cs 2.7 mm, 300 kV, 1.2 A / pixel."""
    t = np.zeros((N, 8))
    t[:, 0] = rng.uniform(1.0, 3.0, N)
    t[:, 1], t[:, 2], t[:, 3] = 2.7, 300.0, 1.2
    t[:, 4] = rng.uniform(*bfactor, N)
    t[:, 5] = ampcont
    t[:, 6], t[:, 7] = rng.uniform(0, 0.1, N), rng.uniform(0, 180, N)      # ignored
    return t


def coef_rows(rng, N, c2_scale=1.0, **kw):
    from tvae import ctf
    c = ctf.coefficients(table(rng, N, **kw))
    c[:, 2] *= c2_scale
    return c


# ---- the C ABI under guard bands ---------------------------------------------------------------------------------------------
def run_eval(coef, n, mode, N=None):
    from tvae import _cluster_lib as CL
    N = coef.shape[0] if N is None else N
    H = torch.full((coef.shape[0], max(n, 1), max(n, 1) // 2 + 1), SENT_F, device=DEV)
    try:
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_ctf_eval', _dev(coef, torch.float64), H, N, n, mode)
    finally:
        run_eval.last = H.cpu().numpy()
    return H.cpu().numpy()


def run_filter(X, n, coef=None, Hp=None, mode=0, B=B_IMG, x_stride=None, h_stride=None, inplace=False, ws_short=0):
    """tvae_fourier_filter with a sentinel-filled output and workspace -> numpy [B][n][n].  X: any array whose flat contents
    are the planes at x_stride (default n n); Hp likewise at h_stride (default n R)."""
    from tvae import _cluster_lib as CL
    R = n // 2 + 1
    x = _dev(np.asarray(X, dtype=np.float32).reshape(-1))
    wsf = CL.query('tvae_fourier_filter_ws_floats', B, n)
    alloc = max(wsf, 2)
    ws = torch.full((alloc // 2,), SENT_F, dtype=torch.float64, device=DEV).view(torch.float32)
    out = x[:B * n * n] if inplace else torch.full((B * n * n,), SENT_F, device=DEV)
    hp = None if Hp is None else _dev(np.asarray(Hp, dtype=np.float32).reshape(-1))
    try:
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_fourier_filter', x, n * n if x_stride is None else x_stride, _dev(coef, torch.float64), hp,
                    n * R if h_stride is None else h_stride, out, ws, alloc - ws_short, B, n, mode)
    finally:
        run_filter.last = (None if inplace else out.cpu().numpy(), ws.cpu().numpy())
    return out.cpu().numpy().reshape(B, n, n)


def run_power(coef, order, seg, n, N=None):
    from tvae import _cluster_lib as CL
    N = coef.shape[0] if N is None else N
    K = len(seg) - 1
    D = torch.full((K, n, n // 2 + 1), SENT_F, dtype=torch.float64, device=DEV)
    counts = torch.full((K,), -7, dtype=torch.int32, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_ctf_power', _dev(coef, torch.float64), _dev(order, torch.int32), _dev(seg, torch.int32), D, counts, N, K,
                n)
    return D.cpu().numpy(), counts.cpu().numpy()


# ---- 1. tvae_ctf_eval ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sign_rows(n, c2_scale):
    """Three rows, found by a seeded search on the CPU, none of whose grid frequencies has |H_fp64| < 1e-3 (the B factors of the
    range that pass are the small ones: the envelope alone must stay above 1e-3 up to the corner of the spectrum)."""
    rng = np.random.default_rng([n, int(c2_scale), 11])
    found = []
    for _ in range(200):
        c = coef_rows(rng, 512, c2_scale)
        ok = np.abs(ctf_ref.H(c, n)).reshape(512, -1).min(1) >= 1e-3
        found += list(c[ok])
        if len(found) >= 3:
            return np.array(found[:3])
    raise AssertionError('no rows found')


@pytest.mark.parametrize('n', (2, 3, 31, 64, 65))
def test_eval_against_the_contract(n):
    rng = np.random.default_rng(100 + n)
    coef = np.concatenate([coef_rows(rng, 4), coef_rows(rng, 4, 50.0)])
    ref = ctf_ref.H(coef, n)
    got = run_eval(coef, n, 0)
    c01 = np.abs(coef[:, 0]) + np.abs(coef[:, 1])
    err = np.abs(got - ref) / (8 * EPS * c01[:, None, None])
    print('value: max error / bound %.3f' % err.max())
    assert got.dtype == np.float32 and err.max() <= 1.0
    # the phase really is many turns in the scaled rows: without the fp64 reduction fp32 would have lost it
    q = ctf_ref.q_grid(n)
    if n >= 31:
        assert np.abs(coef[4:, 2, None, None] * q[None]).max() > 500
    for scale in (1.0, 50.0):
        rows = sign_rows(n, scale)
        ref = ctf_ref.H(rows, n)
        assert np.abs(ref).min() >= 1e-3
        sgn = run_eval(rows, n, 1)
        assert np.array_equal(sgn, ctf_ref.H(rows, n, 1).astype(np.float32)) and set(np.unique(sgn)) <= {-1.0, 1.0}


# ---- 2. tvae_fourier_filter ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, kind, mode):
    """Inputs (seeded until the conditions of the docstring hold), the fp64 reference (computed once, never modified), both
    tolerances and the guarded GPU result."""
    for seed in range(50):
        rng = np.random.default_rng([n, kind == 'plane', mode, seed])
        X = (rng.standard_normal((B_IMG, n, n)) + 0.5).astype(np.float32)
        if kind == 'coef':
            coef, Hp = coef_rows(rng, B_IMG), None
            c01 = np.abs(coef[:, 0]) + np.abs(coef[:, 1])
            value = ctf_ref.H(coef, n)
            if mode == 1 and np.abs(value).min() < 64 * EPS:             # a sign that 8 u (|c0| + |c1|) could turn
                continue
            used = ctf_ref.H(coef, n, mode)
        else:
            coef, Hp = None, rng.standard_normal((B_IMG, n, n // 2 + 1)).astype(np.float32)
            c01 = 0.0
            used = np.where(Hp < 0, -1.0, 1.0) if mode == 1 else Hp.astype(np.float64)
        ref = ctf_ref.filter(X, used)
        bound = ctf_ref.filter_bound(X, used, c01 if mode == 0 else 0.0)
        if (bound <= 1e-2 * np.sqrt((ref ** 2).sum((1, 2)))).all():
            break
    else:
        raise AssertionError('no seed meets the conditions')
    f32 = ctf_ref.filter_f32(X, used.astype(np.float32))
    limit = 8 * np.abs(f32 - ref).max()
    got = run_filter(X, n, coef, Hp, mode)
    for a in (X, ref):
        a.setflags(write=False)
    return dict(X=X, coef=coef, Hp=Hp, used=used, ref=ref, bound=bound, limit=limit, got=got)


@pytest.mark.parametrize('mode', (0, 1), ids=('multiply', 'flip'))
@pytest.mark.parametrize('kind', ('coef', 'plane'))
@pytest.mark.parametrize('n', SIZES)
def test_filter_against_fp64(n, kind, mode):
    c = case(n, kind, mode)
    assert c['got'].shape == c['ref'].shape and np.isfinite(c['got']).all()
    err = c['got'] - c['ref']
    frob = np.sqrt((err ** 2).sum((1, 2)))
    print('(a) max error / bound %.4f   (b) max error / limit %.4f   limit %.3e' % (
        (frob / c['bound']).max(), np.abs(err).max() / c['limit'], c['limit']))
    assert (frob <= c['bound']).all()
    assert np.abs(err).max() <= c['limit']


# ---- 3. properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (31, 64, 129))
def test_filter_properties(n):
    for kind in ('coef', 'plane'):
        c = case(n, kind, 0)
        X, coef, Hp = c['X'], c['coef'], c['Hp']
        assert np.array_equal(run_filter(X, n, coef, Hp), c['got'])                       # a second run
        assert np.array_equal(run_filter(X.copy(), n, coef, Hp, inplace=True), c['got'])  # out == X
        for b in (0, 3):
            one = run_filter(X[b:b + 1], n, None if coef is None else coef[b:b + 1], None if Hp is None else Hp[b:b + 1], B=1)
            assert np.array_equal(one[0], c['got'][b]), (kind, b)
        # one shared plane (x_stride = 0) against five copies of it
        shared = run_filter(X[2], n, coef, Hp, x_stride=0)
        assert np.array_equal(shared, run_filter(np.repeat(X[2:3], B_IMG, 0), n, coef, Hp))
        assert np.array_equal(shared[2], c['got'][2])
    # one shared transfer plane (h_stride = 0) against five copies; H = 1 returns x within (b)
    c = case(n, 'plane', 0)
    assert np.array_equal(run_filter(c['X'], n, Hp=c['Hp'][1], h_stride=0)[1], c['got'][1])
    ones = np.ones((n, n // 2 + 1), dtype=np.float32)
    back = run_filter(c['X'], n, Hp=ones, h_stride=0)
    limit = 8 * np.abs(ctf_ref.filter_f32(c['X'], ones) - c['X'].astype(np.float64)).max()
    print('H = 1: max error / limit %.4f' % (np.abs(back - c['X']).max() / limit))
    assert np.abs(back - c['X']).max() <= limit


# ---- 4. tvae_ctf_power -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (8, 31))
def test_power(n):
    N, K = 40, 4
    rng = np.random.default_rng(400 + n)
    coef = coef_rows(rng, N)
    lab = rng.permutation(np.concatenate([np.zeros(17, int), np.full(14, 1), np.full(9, 3)]))          # no label 2
    order, seg, _ = align_ref.segments(lab, K)
    order = order.copy()
    order[[3, 20, 33]] = [-1, N, 1 << 30]                                # skipped, not counted
    seg = seg.copy()
    seg[2] = seg[1] - 5                                                  # not monotone: cleaned to seg[1] -- class 1 is empty
    seg[4] = N + 9                                                       # clamped to N
    ref, cnt = ctf_ref.power(coef, order, seg, n)
    D, counts = run_power(coef, order, seg, n)
    assert np.array_equal(counts, cnt) and cnt[1] == 0 and cnt[2] > 0 and cnt.sum() == N - 3        # (class 2 takes label 1's)
    c01 = np.abs(coef[:, 0]) + np.abs(coef[:, 1])
    habs = np.abs(ctf_ref.H(coef, n))
    clean = np.minimum(np.maximum.accumulate(np.maximum(seg, 0)), N)
    for k in range(K):
        m = order[clean[k]:clean[k + 1]]
        m = m[(m >= 0) & (m < N)]
        tol = (2 * 8 * EPS * c01[m, None, None] * habs[m]).sum(0) + (m.size + 2) * 2.0 ** -52 * ref[k]
        assert (np.abs(D[k] - ref[k]) <= tol).all(), k
    assert (D[1] == 0).all()
    # class k's bits do not depend on the other classes or on K: classes permuted (0 1 2 3 -> 3 0 1 2), then class 0 alone
    perm = np.array([3, 0, 1, 2])
    lab2 = perm[lab]
    o2, s2, _ = align_ref.segments(lab2, K)
    ref_o, ref_s, _ = align_ref.segments(lab, K)
    D1, c1 = run_power(coef, ref_o, ref_s, n)
    D2, c2 = run_power(coef, o2, s2, n)
    assert np.array_equal(D2[perm], D1) and np.array_equal(c2[perm], c1)
    D3, c3 = run_power(coef, ref_o, ref_s[:2], n)
    assert np.array_equal(D3[0], D1[0]) and c3[0] == c1[0]


# ---- 5. rejections -----------------------------------------------------------------------------------------------------------------
def test_rejections():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    rng = np.random.default_rng(5)
    n = 8
    X = rng.standard_normal((B_IMG, n, n)).astype(np.float32)
    coef = coef_rows(rng, B_IMG)
    Hp = np.ones((B_IMG, n, n // 2 + 1), dtype=np.float32)
    big = np.zeros((1, 1025, 1025), dtype=np.float32)
    bad = [
        dict(X=X[:, :1, :1], n=1, coef=coef),
        dict(X=big, n=1025, coef=coef[:1], B=1),
        dict(X=X, n=n, coef=coef, Hp=Hp),                                 # both
        dict(X=X, n=n),                                                  # neither
        dict(X=X, n=n, coef=coef, x_stride=n * n - 1),
        dict(X=X, n=n, coef=coef, x_stride=1),
        dict(X=X, n=n, Hp=Hp, h_stride=n * (n // 2 + 1) - 1),
        dict(X=X, n=n, coef=coef, ws_short=1),
        dict(X=X, n=n, coef=coef, mode=2),
        dict(X=X, n=n, coef=coef, mode=-1),
        dict(X=X, n=n, coef=coef, B=0),
    ]
    for kw in bad:
        with pytest.raises(TvaeHipError, match='hipError_t 1'):
            run_filter(**kw)
        out, ws = run_filter.last
        assert (out == SENT_F).all() and np.array_equal(ws.view(np.float64), np.full(ws.size // 2, SENT_F)), kw
    # the workspace route: one float short
    Xb = rng.standard_normal((2, 129, 129)).astype(np.float32)
    assert CL.query('tvae_fourier_filter_ws_floats', 2, 129) == 2 * 4 * 129 * 65
    assert CL.query('tvae_fourier_filter_ws_floats', 2, 128) == 2
    with pytest.raises(TvaeHipError, match='hipError_t 1'):
        run_filter(Xb, 129, coef[:2], B=2, ws_short=1)
    out, ws = run_filter.last
    assert (out == SENT_F).all() and np.array_equal(ws.view(np.float64), np.full(ws.size // 2, SENT_F))
    for args in [(0, 8), (5, 1), (5, 1025), ((1 << 24) + 1, 8), (-1, 8)]:
        assert CL.query('tvae_fourier_filter_ws_floats', *args) == 0
    # out inside X without being X plane over plane: rejected (the guard keeps the two arguments in one allocation)
    x = _dev(X.reshape(-1))
    before = x.clone()
    ws = torch.full((1,), SENT_F, dtype=torch.float64, device=DEV).view(torch.float32)
    with pytest.raises(TvaeHipError, match='hipError_t 1'):
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_fourier_filter', x, n * n, _dev(coef[:2], torch.float64), None, 0, x[n * n:3 * n * n], ws, 2, 2, n, 0)
    assert torch.equal(x, before)
    # a coefficient pointer that is not 8-byte aligned.  torch cannot form such a float64 tensor, so this one call goes to the
    # library directly: it is refused before anything is launched
    c = _dev(np.concatenate([coef.reshape(-1), [0.0]]), torch.float64)
    xg, out = _dev(X), torch.full((B_IMG, n, n), SENT_F, device=DEV)
    rc = CL.lib().tvae_fourier_filter(xg.data_ptr(), n * n, c.data_ptr() + 4, None, 0, out.data_ptr(), ws.data_ptr(), 2, B_IMG,
                                      n, 0, torch.cuda.current_stream().cuda_stream)
    H = torch.full((B_IMG, n, n // 2 + 1), SENT_F, device=DEV)
    rc2 = CL.lib().tvae_ctf_eval(c.data_ptr() + 4, H.data_ptr(), B_IMG, n, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 1 and rc2 == 1 and (out == SENT_F).all() and (H == SENT_F).all()
    # tvae_ctf_eval and tvae_ctf_power
    for kw in (dict(n=1), dict(n=1025), dict(n=8, mode=2), dict(n=8, N=0)):
        with pytest.raises(TvaeHipError, match='hipError_t 1'):
            run_eval(coef, kw['n'], kw.get('mode', 0), kw.get('N'))
        assert (run_eval.last == SENT_F).all()
    order, seg, _ = align_ref.segments(np.zeros(B_IMG, int), 1)
    for kw in (dict(n=1), dict(n=1025), dict(n=8, N=0)):
        with pytest.raises(TvaeHipError, match='hipError_t 1'):
            run_power(coef, order, seg, kw['n'], kw.get('N'))


# ---- 6. filter_bank against the reference's own filters ------------------------------------------------------------------------------
def test_filter_bank_reproduces_the_reference():
    from tvae import ctf
    fx = load_golden('ctf_filters')
    n = int(fx['n'])
    params = np.stack([fx[c] for c in ctf.COLUMNS], 1)
    want = fx['filters']
    assert n == 31 and want.shape == (params.shape[0], n, n) and want.dtype == np.float32
    with guardband.GuardedCalls(replay=True):
        got = ctf.filter_bank(params, n).cpu().numpy()
    delta = np.zeros((1, n, n))
    delta[0, n // 2, n // 2] = 1.0
    coef = ctf.coefficients(params)
    Hh = ctf_ref.H(coef, n)
    ref = ctf_ref.filter(delta, Hh)
    tol = ctf_ref.filter_bound(np.repeat(delta, len(coef), 0), Hh, np.abs(coef[:, 0]) + np.abs(coef[:, 1]))
    tol = tol + EPS * np.sqrt((want.astype(np.float64) ** 2).sum((1, 2)))
    err = np.sqrt(((got - want.astype(np.float64)) ** 2).sum((1, 2)))
    print('max error / tolerance %.4f' % (err / tol).max())
    assert got.shape == want.shape and (err <= tol).all()
    assert np.abs(ref - want).max() <= 1e-6 * np.abs(want).max()          # (the fixture is what the definitions give)
    # an even size as well: -fftshift(Re ifft2(c)), against src.ctf itself
    import pandas as pd
    import src.ctf as C
    host = C.ctf_filter(pd.DataFrame({c: fx[c] for c in ctf.COLUMNS}), 32, 32)
    with guardband.GuardedCalls(replay=True):
        even = ctf.filter_bank(params, 32).cpu().numpy()
    d32 = np.zeros((len(coef), 32, 32))
    d32[:, 16, 16] = 1.0
    tol = ctf_ref.filter_bound(d32, ctf_ref.H(coef, 32), np.abs(coef[:, 0]) + np.abs(coef[:, 1]))
    tol = tol + EPS * np.sqrt((host.astype(np.float64) ** 2).sum((1, 2)))
    assert (np.sqrt(((even - host.astype(np.float64)) ** 2).sum((1, 2))) <= tol).all()


# ---- 7. class_averages_ctf -------------------------------------------------------------------------------------------------------------
def smooth_image(rng, n, blobs=6):
    """A zero-mean sum of Gaussian blobs inside the central disc."""
    yy, xx = np.mgrid[:n, :n].astype(np.float64)
    img = np.zeros((n, n))
    for _ in range(blobs):
        cy, cx = rng.uniform(0.3 * n, 0.7 * n, 2)
        s = rng.uniform(0.06 * n, 0.12 * n)
        img += rng.uniform(0.5, 1.5) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return img - img.mean()


def column_sums(n, theta, dx, t):
    """c_i [N]: the largest column sum of image i's bilinear alignment matrix (its row sums are at most 1)."""
    col, row = align_ref.positions(n, theta, dx, t)
    N = col.shape[0]
    inside = (col > -1) & (col < n) & (row > -1) & (row < n)
    col, row = np.where(inside, col, 0.0), np.where(inside, row, 0.0)
    c0, r0 = np.floor(col).astype(np.int64), np.floor(row).astype(np.int64)
    wc, wr = col - c0, row - r0
    acc = np.zeros((N, n + 2, n + 2))
    ii = np.broadcast_to(np.arange(N)[:, None, None], col.shape)
    for dr, dc, w in ((0, 0, (1 - wr) * (1 - wc)), (0, 1, (1 - wr) * wc), (1, 0, wr * (1 - wc)), (1, 1, wr * wc)):
        np.add.at(acc, (ii, r0 + 1 + dr, c0 + 1 + dc), np.where(inside, w, 0.0))
    return acc[:, 1:-1, 1:-1].max((1, 2))


@pytest.mark.parametrize('correct', ('wiener', 'flip'))
@pytest.mark.parametrize('n', (31, 32))
def test_class_averages_ctf(n, correct):
    from test_align_gpu import average_bounds, image_bounds
    from tvae import ctf
    N, K, C, tau, t = 40, 3, 1, 0.1, 1.0
    rng = np.random.default_rng(700 + n)
    coef = coef_rows(rng, N, bfactor=(0.0, 0.0), ampcont=60.0)            # mean H^2 stays away from 0: max G about 3
    c01 = np.abs(coef[:, 0]) + np.abs(coef[:, 1])
    lab = rng.permutation(np.concatenate([np.zeros(22, int), np.full(18, 2)]))              # class 1 is empty
    theta = rng.uniform(-np.pi, np.pi, N).astype(np.float32)
    dx = rng.uniform(-0.15, 0.15, (N, 2)).astype(np.float32)
    base = [smooth_image(rng, n) for _ in range(K)]
    # every particle: its class's image, rotated and shifted by the inverse of its pose (to fp64), CTF-filtered, plus noise
    raw = np.stack([base[k] for k in lab])[:, None]
    inv = align_ref.align_stack(raw, -theta.astype(np.float64), np.zeros((N, 2)), t)
    Y = (ctf_ref.filter(inv, ctf_ref.H(coef, n)[:, None]) + 0.005 * rng.standard_normal((N, C, n, n))).astype(np.float32)
    ref, cnt, Dref = ctf_ref.class_averages_ctf(Y, theta, dx, lab, coef, K, t, correct, tau)
    with guardband.GuardedCalls(replay=True):
        avg, counts, D = ctf.class_averages_ctf(_dev(Y), _dev(theta), _dev(dx), lab, coef, K, t, correct, tau)
    avg, counts, D = avg.cpu().numpy(), counts.cpu().numpy(), D.cpu().numpy()
    assert avg.shape == (K, C, n, n) and np.array_equal(counts, cnt) and (avg[1] == 0).all() and (D[1] == 0).all()
    assert np.abs(D - Dref).max() <= 2 * 8 * EPS * c01.max() * 1.1 * 22 + 1e-12
    # the tolerance of the docstring
    mode = 1 if correct == 'flip' else 0
    Hused = ctf_ref.H(coef, n, mode)
    a = ctf_ref.filter_bound(Y[:, 0], Hused, c01 if mode == 0 else 0.0)
    xf = ctf_ref.filter(Y, Hused[:, None])
    aligned = align_ref.align_stack(xf, theta, dx, t)
    order, seg, _ = align_ref.segments(lab, K)
    mean, _ = align_ref.class_averages(aligned, order, seg)
    avb = average_bounds(aligned, image_bounds(xf, dx, t), order, seg)
    csum = np.sqrt(column_sums(n, theta, dx, t))
    for k in (0, 2):
        m = np.flatnonzero(lab == k)
        tol = (csum[m] * a[m]).mean() + np.sqrt((avb[k] ** 2).sum())
        if correct == 'wiener':
            G = 1.0 / (Dref[k] / m.size + tau)
            rel_g = EPS + 16 * EPS * c01[m].max() * np.abs(Hused[m]).max() / tau
            tol = G.max() * tol + rel_g * G.max() * np.sqrt((mean[k] ** 2).sum())
            tol += ctf_ref.filter_bound(mean[k], G.astype(np.float32).astype(np.float64))[0]
        nref = np.sqrt((ref[k] ** 2).sum())
        err = np.sqrt(((avg[k] - ref[k]) ** 2).sum())
        print('class %d: tolerance / |ref| %.3e, error / tolerance %.4f' % (k, tol / nref, err / tol))
        assert tol <= 1e-3 * nref
        assert err <= tol


# ---- 8. recovery ---------------------------------------------------------------------------------------------------------------------
def recovery_inputs(n=32, members=16):
    rng = np.random.default_rng(8)
    S = smooth_image(rng, n)
    tab = table(rng, members, bfactor=(0.0, 0.0))
    tab[:, 0] = np.linspace(1.0, 3.0, members)
    from tvae import ctf
    coef = ctf.coefficients(tab)
    X = ctf_ref.filter(np.repeat(S[None], members, 0), ctf_ref.H(coef, n)).astype(np.float32)[:, None]
    return S, coef, X


def test_wiener_average_recovers_the_image():
    """16 copies of one smooth zero-mean image, each seen through the CTF of its own defocus (1 .. 3 um): the Wiener average gets
    it back to 2 %, the plain average of the same particles is at least five times further away."""
    from tvae import align, ctf
    S, coef, X = recovery_inputs()
    N, n = X.shape[0], X.shape[-1]
    theta, dx, lab = np.zeros(N, np.float32), np.zeros((N, 2), np.float32), np.zeros(N, int)
    nS = np.sqrt((S ** 2).sum())
    ref, _, _ = ctf_ref.class_averages_ctf(X, theta, dx, lab, coef, 1, 1.0, 'wiener', 1e-3)
    assert np.sqrt(((ref[0, 0] - S) ** 2).sum()) <= 0.01 * nS              # the reference alone: well inside
    with guardband.GuardedCalls(replay=True):
        avg, counts, _ = ctf.class_averages_ctf(_dev(X), _dev(theta), _dev(dx), lab, coef, 1, 1.0, 'wiener', 1e-3)
        plain, _ = align.class_averages(_dev(X), _dev(theta), _dev(dx), lab, 1, 1.0)
    e_w = np.sqrt(((avg.cpu().numpy()[0, 0] - S) ** 2).sum()) / nS
    e_p = np.sqrt(((plain.cpu().numpy()[0, 0] - S) ** 2).sum()) / nS
    print('wiener %.4f, plain %.4f of |S|' % (e_w, e_p))
    assert int(counts[0]) == N and e_w <= 0.02 and e_p >= 5 * e_w


# ---- 9. command lines ----------------------------------------------------------------------------------------------------------------
def test_command_lines(tmp_path):
    from tvae import align, ctf, resolution
    N, n, K = 40, 16, 3
    rng = np.random.default_rng(9)
    stack = rng.standard_normal((N, n, n)).astype(np.float32)
    theta = rng.uniform(-np.pi, np.pi, N).astype(np.float32)
    dx = rng.uniform(-0.2, 0.2, (N, 2)).astype(np.float32)
    lab = rng.integers(0, K, N)
    tab = table(rng, N)
    files = {}
    for name, arr in (('stack', stack), ('rotations', theta), ('translations', dx), ('clusters', lab)):
        files[name] = str(tmp_path / (name + '.npy'))
        np.save(files[name], arr)
    ctf_file = str(tmp_path / 'ctf.txt')
    np.savetxt(ctf_file, tab)
    common = ['--stack', files['stack'], '--rotations', files['rotations'], '--translations', files['translations'],
              '--clusters', files['clusters']]

    def run(script, out, extra):
        os.makedirs(out)
        r = subprocess.run([sys.executable, os.path.join(PKG, script)] + common + ['--out-dir', out] + extra,
                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]

    # the runs without --ctf: the same entry points in this process (the scripts only call them)
    a0, a1 = str(tmp_path / 'avg0'), str(tmp_path / 'avg1')
    with guardband.GuardedCalls(replay=True):
        align.run(common + ['--out-dir', a0])
    run('class_averages.py', a1, ['--ctf', ctf_file, '--ctf-correct', 'wiener', '--wiener-tau', '0.2', '--scale', '2'])
    for f in sorted(os.listdir(a0)):
        assert open(os.path.join(a0, f), 'rb').read() == open(os.path.join(a1, f), 'rb').read(), f
    assert set(os.listdir(a1)) - set(os.listdir(a0)) >= {'class_averages_ctf.npy', 'class_ctf_power.npy'}
    got = np.load(os.path.join(a1, 'class_averages_ctf.npy'))
    power = np.load(os.path.join(a1, 'class_ctf_power.npy'))
    assert got.shape == (K, 1, n, n) and got.dtype == np.float32 and power.shape == (K, n, n // 2 + 1)
    coef = ctf.coefficients(tab, scale=2)
    with guardband.GuardedCalls(replay=True):
        want, _, D = ctf.class_averages_ctf(_dev(stack[:, None]), _dev(theta), _dev(dx), lab, coef, None, 1.0, 'wiener', 0.2)
    assert np.array_equal(got, want.cpu().numpy()) and np.array_equal(power, D.cpu().numpy())
    r0, r1 = str(tmp_path / 'res0'), str(tmp_path / 'res1')
    with guardband.GuardedCalls(replay=True):
        resolution.run(common + ['--out-dir', r0])
    run('class_resolution.py', r1, ['--ctf', ctf_file, '--ctf-correct', 'flip'])
    assert sorted(os.listdir(r0)) == sorted(os.listdir(r1))
    with guardband.GuardedCalls(replay=True):
        flipped = ctf.filter_stack(_dev(stack[:, None]), coef=ctf.coefficients(tab), mode='flip')
        _, halves, var, counts = align.class_halves(flipped, _dev(theta), _dev(dx), lab, None, 1.0)
    assert np.array_equal(np.load(os.path.join(r1, 'class_halves.npy')), halves.cpu().numpy())
    assert np.array_equal(np.load(os.path.join(r1, 'class_variance.npy')), var.cpu().numpy())
    assert np.array_equal(np.load(os.path.join(r1, 'class_counts.npy')), np.load(os.path.join(r0, 'class_counts.npy')))
    assert not np.array_equal(np.load(os.path.join(r1, 'class_halves.npy')), np.load(os.path.join(r0, 'class_halves.npy')))


# ---- 10. the training driver's switch ------------------------------------------------------------------------------------------------
def test_driver_builds_the_filter_bank_on_the_gpu_when_asked(tmp_path, monkeypatch):
    """TVAE_CTF_GPU=1: driver._load_ctf returns tvae.ctf.filter_bank's filters, equal to the host's within bound (a) and the
    fp32 rounding of the host's own; unset, it is the host path."""
    import types
    from tvae import ctf, driver
    rng = np.random.default_rng(10)
    tab = table(rng, 7)
    path = str(tmp_path / 'ctf.txt')
    np.savetxt(path, tab)
    args = types.SimpleNamespace(ctf_train=path, ctf_test=None, scale=2)
    monkeypatch.delenv('TVAE_CTF_GPU', raising=False)
    host_tr, host_te = driver._load_ctf(args, 5, 2, 32)
    monkeypatch.setenv('TVAE_CTF_GPU', '1')
    with guardband.GuardedCalls(replay=True):
        gpu_tr, gpu_te = driver._load_ctf(args, 5, 2, 32)
    assert gpu_tr.shape == host_tr.shape == (5, 1, 31, 31) and gpu_te.shape == host_te.shape == (2, 1, 31, 31)
    assert gpu_tr.dtype == torch.float32 and not gpu_tr.is_cuda
    coef = ctf.coefficients(tab, scale=2)
    delta = np.zeros((7, 31, 31))
    delta[:, 15, 15] = 1.0
    host = torch.cat([host_tr, host_te])[:, 0].numpy().astype(np.float64)
    got = torch.cat([gpu_tr, gpu_te])[:, 0].numpy().astype(np.float64)
    tol = ctf_ref.filter_bound(delta, ctf_ref.H(coef, 31), np.abs(coef[:, 0]) + np.abs(coef[:, 1]))
    tol = tol + EPS * np.sqrt((host ** 2).sum((1, 2)))
    assert (np.sqrt(((got - host) ** 2).sum((1, 2))) <= tol).all()
