"""Maximum-likelihood class averages on the GPU: tvae_pose_posterior and tvae_class_average_weighted behind their C ABI (every
call under guard bands with replay, outputs and workspace filled with a sentinel) against the fp64 restatement
tests/ml_ref.py, and tvae.ml2d.ml_rounds on a noisy planted stack.

Posterior: everything is fp64 on the device as in the reference, so indices and classes are exact, the poses bit-equal, the
weights within an fp32 rounding and lse / r2 within 1e-12 relative (the exp, the log and the order of the sums differ).
Weighted average: per pixel  sum w_e b_e / W + (min(E_k, chunk) + 2) 2^-24 sum w_e |A_e| / W,  b_e the per-image bound of
test_align_gpu.py at the entry's dx (ml_ref.image_bounds), the second term the fp32 chain of a chunk, the division and the
rounding of the result."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref
import guardband
import ml_ref
import pose_ref
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32 = np.float32
EPS = 2.0 ** -24
SENT_F, SENT_I = -12345.5, -777


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


# ---- the posterior ---------------------------------------------------------------------------------------------------------------
# (M, A, S, P): J = 1, 81, 1125 and 6, whose log weights stay in LDS; then the two sides of that cache's 4 096 candidates
# (J = M NA NS^2 is M times an odd number: 4 095 = 63 x 65 is the nearest below or at it, 4 100 = 4 x 41 x 25 the nearest above),
# and J = 4 250, all K = 10 classes at the command line's default A = 8, S = 2: the last two form every log weight again where
# it is needed
POST_SHAPES = [(1, 0, 0, 1), (3, 1, 1, 16), (5, 4, 2, 8), (2, 1, 0, 64), (63, 32, 0, 8), (4, 20, 2, 8), (10, 8, 2, 8)]
POST_CACHE = 4096
POST_N, POST_n, POST_T, POST_DTH, POST_S2 = 6, 16, 0.5, 0.037, 30.0


def post_classes(M):
    """K of a shape: M distinct classes with prior mass for every row, and one class without."""
    return max(7, M + 2)


def run_posterior(c, rows=None, sigma2=POST_S2):
    """tvae_pose_posterior on the images `rows` of case c into sentinel-filled outputs -> dict of numpy arrays."""
    from tvae import _cluster_lib as CL
    rows = np.arange(POST_N) if rows is None else np.asarray(rows)
    N, (M, A, S, P) = rows.size, c['shape']
    out = dict(idx=torch.full((N, P), SENT_I, dtype=torch.int32, device=DEV), cls=torch.full((N, P), SENT_I, dtype=torch.int32, device=DEV),
               theta=torch.full((N, P), SENT_F, device=DEV), dx=torch.full((N, P, 2), SENT_F, device=DEV),
               w=torch.full((N, P), SENT_F, device=DEV), resp=torch.full((N, M), SENT_F, device=DEV),
               lse=torch.full((N,), SENT_F, dtype=torch.float64, device=DEV), r2=torch.full((N,), SENT_F, dtype=torch.float64, device=DEV),
               kept=torch.full((N,), SENT_F, device=DEV))
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_posterior', _dev(c['num'][rows]), _dev(c['pp'][rows]), _dev(c['yy'][rows]), _dev(c['cand'][rows], torch.int32),
                _dev(c['lp'], torch.float64), _dev(c['theta'][rows]), _dev(c['dx'][rows]), out['idx'], out['cls'], out['theta'],
                out['dx'], out['w'], out['resp'], out['lse'], out['r2'], out['kept'], N, POST_n, c['K'], M, A, S, P, POST_T,
                POST_DTH, sigma2)
    return {k: v.cpu().numpy() for k, v in out.items()}


def post_inputs(shape):
    """Random tables for six images: 0 plain (one invalid slot where M > 1), 1 with every slot invalid, 2 with a NaN in num, 3
    with a -inf prior on its only class, 4 with two bit-identical candidates of one slot at the top (J > 1), 5 with tables so
    large that every weight but the first underflows to 0; and the fp64 reference."""
    M, A, S, P = shape
    rng = np.random.default_rng(100 * M + 10 * A + S)
    NA, NS = 2 * A + 1, 2 * S + 1
    J = M * NA * NS * NS
    N, K = POST_N, post_classes(M)
    pp = rng.uniform(50, 150, (N, M, NA, NS, NS)).astype(F32)
    yy = rng.uniform(100, 200, N).astype(F32)
    num = rng.uniform(-40, 90, (N, M, NA, NS, NS)).astype(F32)
    cand = np.stack([rng.permutation(K - 1)[:M] for _ in range(N)])           # classes 0 .. K - 2, distinct within a row
    lp = np.log(rng.dirichlet(np.ones(K - 1)))
    lp = np.concatenate([lp, [-np.inf]])                                        # class K - 1 has no prior mass
    if M > 1:
        cand[0, 1] = K
    cand[1] = np.resize([-1, K, -5, K + 3, -1], M)
    num.reshape(N, -1)[2, J // 2] = np.nan
    cand[3] = -1
    cand[3, M - 1] = K - 1
    pair = None
    if J > 1:
        cnd = NA * NS * NS
        pair = (J - 1 - max(1, cnd // 2), J - 1)                                # both in the last slot: one prior
        num.reshape(N, -1)[4, list(pair)] = 1000.0                              # far above every other num: the two best
        pp.reshape(N, -1)[4, list(pair)] = 50.0
    num[5], pp[5], yy[5] = num[5] * F32(1e9), pp[5] * F32(1e9), yy[5] * F32(1e9)
    theta = rng.uniform(-3, 3, N).astype(F32)
    dx = rng.uniform(-0.4, 0.4, (N, 2)).astype(F32)
    c = dict(shape=shape, J=J, K=K, num=num, pp=pp, yy=yy, cand=cand, lp=lp, theta=theta, dx=dx, pair=pair)
    c['ref'] = ml_ref.posterior(num, pp, yy, cand, lp, theta, dx, POST_n, K, A, S, P, POST_T, POST_DTH, POST_S2)
    return c


@functools.lru_cache(maxsize=None)
def post_case(shape):
    """The inputs, the reference (computed once, never modified) and the guarded GPU results of one shape."""
    c = post_inputs(shape)
    c['got'] = run_posterior(c)
    for v in list(c.values()) + list(c['ref'].values()) + list(c['got'].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize('shape', POST_SHAPES)
def test_posterior_inputs_are_separated(shape):
    """Apart from the planted pair, the reference's l within an image are 1e-9 |l| apart: contraction cannot change the ranking."""
    c = post_case(shape)
    l = c['ref']['l'].copy()
    if c['pair']:
        assert l[4, c['pair'][0]] == l[4, c['pair'][1]]                        # bit-identical
        l[4, c['pair'][1]] = np.nan
    sep, tie = ml_ref.separation(l)
    print(f'posterior {shape}: least relative separation {sep.min():.3e}')
    assert not tie.any() and (sep >= 1e-9).all()
    assert c['ref']['live'].tolist() == [True, False, c['J'] > 1, False, True, True]


@pytest.mark.parametrize('shape', POST_SHAPES)
def test_posterior_against_fp64(shape):
    c = post_case(shape)
    ref, got = c['ref'], c['got']
    M, A, S, P = shape
    for k, v in got.items():
        assert not (v == (SENT_I if v.dtype == np.int32 else SENT_F)).any(), k
    assert np.array_equal(got['idx'], ref['idx']) and np.array_equal(got['cls'], ref['cls'])
    assert got['theta'].tobytes() == ref['theta'].tobytes() and got['dx'].tobytes() == ref['dx'].tobytes()
    for key, want in (('w', ref['w']), ('resp', ref['resp']), ('kept', ref['kept'])):
        err = np.abs(got[key].astype(np.float64) - want)
        tol = 2.0 ** -23 * want + 1e-12
        print(f'posterior {shape} {key}: worst error / bound {(err / tol).max():.3f}')
        assert (err <= tol).all(), key
    live = ref['live']
    for key in ('lse', 'r2'):
        rel = np.abs(got[key][live] - ref[key][live]) / np.abs(ref[key][live])
        print(f'posterior {shape} {key}: worst relative error {rel.max() if rel.size else 0.0:.3e}')
        assert (rel <= 1e-12).all(), key
    # dead images and empty ranks exactly as specified
    for i in np.flatnonzero(~live):
        assert got['lse'][i] == 0 and got['r2'][i] == 0 and got['kept'][i] == 0 and not got['resp'][i].any()
        assert (got['idx'][i] == -1).all() and (got['cls'][i] == -1).all() and not got['w'][i].any()
    empty = got['idx'] < 0
    assert np.array_equal(empty, got['cls'] < 0) and not got['w'][empty].any()
    own_th, own_dx = np.repeat(c['theta'][:, None], P, 1), np.repeat(c['dx'][:, None, :], P, 1)
    assert got['theta'][empty].tobytes() == own_th[empty].tobytes() and got['dx'][empty].tobytes() == own_dx[empty].tobytes()
    assert (empty.sum(1) == np.maximum(P - (~np.isnan(ref['l'])).sum(1), 0)).all()
    if c['pair']:                                             # the tie goes to the lower j
        assert got['idx'][4, 0] == c['pair'][0] and got['idx'][4, 1] == c['pair'][1] and got['w'][4, 0] == got['w'][4, 1]
    # image 5: the ranking by l holds although every weight but the first is an exact 0
    assert got['w'][5, 0] == 1.0 and not got['w'][5, 1:].any() and got['kept'][5] == 1.0
    assert not ref['wj'][5, 1:].any() and np.array_equal(got['idx'][5], ref['idx'][5])
    if c['J'] > 1:
        assert (got['idx'][5, :min(P, c['J'])] >= 0).all()


@pytest.mark.parametrize('shape', POST_SHAPES)
def test_posterior_is_reproducible_and_an_image_stands_alone(shape):
    c = post_case(shape)
    again = run_posterior(c)
    for k, v in c['got'].items():
        assert again[k].tobytes() == v.tobytes(), k
    for i in range(POST_N):
        alone = run_posterior(c, [i])
        for k, v in c['got'].items():
            assert alone[k][0].tobytes() == v[i].tobytes(), (i, k)
    sub = run_posterior(c, [4, 0, 5])
    for k, v in c['got'].items():
        assert sub[k].tobytes() == v[[4, 0, 5]].tobytes(), k


@pytest.mark.parametrize('shape', [(5, 4, 2, 8), (10, 8, 2, 8)])
def test_posterior_small_sigma2_and_null_prior(shape):
    """sigma2 small enough that every weight but the first underflows for every image, and logprior = NULL meaning 0; with
    the log weights in LDS and without."""
    from tvae import _cluster_lib as CL
    c = post_case(shape)
    assert (c['J'] > POST_CACHE) == (shape[0] == 10)
    got = run_posterior(c, sigma2=1e-4)
    ref = ml_ref.posterior(c['num'], c['pp'], c['yy'], c['cand'], c['lp'], c['theta'], c['dx'], POST_n, c['K'], *shape[1:], POST_T,
                           POST_DTH, 1e-4)
    assert np.array_equal(got['idx'], ref['idx']) and (got['idx'][0] >= 0).all()
    assert got['w'][0, 0] == 1.0 and not got['w'][0, 1:].any()
    live = ref['live']
    assert (np.abs(got['lse'][live] - ref['lse'][live]) <= 1e-12 * np.abs(ref['lse'][live])).all()
    M, A, S, P = c['shape']
    N = POST_N
    outs = [torch.full((N, P), SENT_I, dtype=torch.int32, device=DEV), torch.full((N, P), SENT_I, dtype=torch.int32, device=DEV),
            torch.full((N, P), SENT_F, device=DEV), torch.full((N, P, 2), SENT_F, device=DEV), torch.full((N, P), SENT_F, device=DEV),
            torch.full((N, M), SENT_F, device=DEV), torch.full((N,), SENT_F, dtype=torch.float64, device=DEV),
            torch.full((N,), SENT_F, dtype=torch.float64, device=DEV), torch.full((N,), SENT_F, device=DEV)]
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_posterior', _dev(c['num']), _dev(c['pp']), _dev(c['yy']), _dev(c['cand'], torch.int32), None,
                _dev(c['theta']), _dev(c['dx']), *outs, N, POST_n, c['K'], M, A, S, P, POST_T, POST_DTH, POST_S2)
    ref0 = ml_ref.posterior(c['num'], c['pp'], c['yy'], c['cand'], None, c['theta'], c['dx'], POST_n, c['K'], A, S, P, POST_T,
                            POST_DTH, POST_S2)
    assert ref0['live'][3]                                    # without the -inf prior image 3 is live
    assert np.array_equal(outs[0].cpu().numpy(), ref0['idx']) and np.array_equal(outs[1].cpu().numpy(), ref0['cls'])
    assert (np.abs(outs[6].cpu().numpy() - ref0['lse'])[ref0['live']] <= 1e-12 * np.abs(ref0['lse'][ref0['live']])).all()


def test_posterior_rejects_unsupported_arguments_and_writes_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    c = post_case((3, 1, 1, 16))
    M, A, S, P = c['shape']
    N = POST_N
    ins = [_dev(c['num']), _dev(c['pp']), _dev(c['yy']), _dev(c['cand'], torch.int32), _dev(c['lp'], torch.float64), _dev(c['theta']),
           _dev(c['dx'])]
    outs = [torch.full((N, P), SENT_I, dtype=torch.int32, device=DEV), torch.full((N, P), SENT_I, dtype=torch.int32, device=DEV),
            torch.full((N, P), SENT_F, device=DEV), torch.full((N, P, 2), SENT_F, device=DEV), torch.full((N, P), SENT_F, device=DEV),
            torch.full((N, M), SENT_F, device=DEV), torch.full((N + 1,), SENT_F, dtype=torch.float64, device=DEV),
            torch.full((N,), SENT_F, dtype=torch.float64, device=DEV), torch.full((N,), SENT_F, device=DEV)]
    good = dict(N=N, n=POST_n, K=c['K'], M=M, A=A, S=S, P=P, t=POST_T, dth=POST_DTH, s2=POST_S2)
    bad = [dict(N=0), dict(n=1), dict(n=129), dict(K=0), dict(K=65536), dict(M=0), dict(M=65), dict(A=-1), dict(A=33), dict(S=-1),
           dict(S=9), dict(P=0), dict(P=65), dict(t=0.0), dict(t=float('nan')), dict(dth=float('inf')), dict(s2=0.0), dict(s2=-1.0),
           dict(s2=float('nan')), dict(s2=float('inf'))]
    for over in bad:
        a = dict(good, **over)
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():                   # a rejected call must leave every tensor as it was
                CL.call('tvae_pose_posterior', *ins, *outs[:6], outs[6][:N], *outs[7:], a['N'], a['n'], a['K'], a['M'], a['A'],
                        a['S'], a['P'], a['t'], a['dth'], a['s2'])
    scal = [good[k] for k in ('N', 'n', 'K', 'M', 'A', 'S', 'P', 't', 'dth', 's2')]
    with pytest.raises(TvaeHipError):                         # resp over cand: an output over an input
        with guardband.GuardedCalls():
            CL.call('tvae_pose_posterior', *ins, *outs[:5], ins[3].view(torch.float32), outs[6][:N], *outs[7:], *scal)
    with pytest.raises(TvaeHipError):                         # no ent_w
        with guardband.GuardedCalls():
            CL.call('tvae_pose_posterior', *ins, *outs[:4], None, outs[5], outs[6][:N], *outs[7:], *scal)
    for o in outs:
        assert (o == (SENT_I if o.dtype == torch.int32 else SENT_F)).all()


# ---- the weighted average -----------------------------------------------------------------------------------------------------------
WAVG_N, WAVG_K = 12, 4
WAVG_GEOMETRIES = [(n, C) for n in (5, 17) for C in (1, 2)]


def run_weighted(Y, img, theta_e, dx_e, w, seg, t):
    """tvae_class_average_weighted with sentinel-filled outputs and workspace -> (avg, wsum, counts) numpy."""
    from tvae import _cluster_lib as CL
    N, C, n, _ = Y.shape
    E, K = len(img), len(seg) - 1
    wsf = CL.query('tvae_class_average_weighted_ws_floats', E, K, C, n)
    assert wsf > 0
    ws = CL.workspace(wsf, DEV)
    ws.fill_(SENT_F)
    avg = torch.full((K, C, n, n), SENT_F, device=DEV)
    wsum = torch.full((K,), SENT_F, dtype=torch.float64, device=DEV)
    counts = torch.full((K,), SENT_I, dtype=torch.int32, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_class_average_weighted', _dev(Y), _dev(img, torch.int32), _dev(theta_e), _dev(dx_e), _dev(w), _dev(seg, torch.int32),
                avg, wsum, counts, ws, wsf, N, E, C, n, K, t)
    return avg.cpu().numpy(), wsum.cpu().numpy(), counts.cpu().numpy()


@functools.lru_cache(maxsize=None)
def wavg_case(n, C):
    """Class 0: 2 chunk + 3 entries (three chunks, the last partial), several of one image at different poses; class 1: one
    entry; class 2: empty; class 3: 40 entries, dead ones (img = -1, img = N, w = 0, -1, NaN, +inf) and live ones with NaN and
    huge poses among them.  C = 1 runs at t = 1, C = 2 at t = 0.1 with the translations scaled by 10."""
    from tvae import _cluster_lib as CL
    rng = np.random.default_rng(1000 * n + C)
    t = 1.0 if C == 1 else 0.1
    N, K = WAVG_N, WAVG_K
    chunk = CL.query('tvae_class_average_weighted_chunk', 300, K, C, n)
    assert chunk > 0
    sizes = [2 * chunk + 3, 1, 0, 40]
    E = sum(sizes)
    seg = np.concatenate([[0], np.cumsum(sizes)])
    Y = rng.standard_normal((N, C, n, n)).astype(F32)
    img = np.concatenate([np.sort(rng.integers(0, N, s)) for s in sizes]).astype(np.int64)       # adjacent entries of one image
    theta = rng.uniform(-np.pi, np.pi, E).astype(F32)
    dx = (rng.uniform(-0.5, 0.5, (E, 2)) / t).astype(F32)
    w = rng.uniform(0.01, 1.0, E).astype(F32)
    w[seg[1]] = 0.75                                          # the class of one
    s3 = seg[3]
    img[s3 + 1], img[s3 + 2] = -1, N
    w[s3 + 4], w[s3 + 5], w[s3 + 6], w[s3 + 7] = 0.0, -1.0, np.nan, np.inf
    theta[s3 + 9], theta[s3 + 10] = np.nan, np.inf
    dx[s3 + 12], dx[s3 + 13], dx[s3 + 14] = (1e30, 0.0), (0.0, -np.inf), (np.nan, 0.1)
    dx[s3 + 15] = (3.0 / t, 0.0)                              # out of frame by a finite pose
    theta[s3 + 6], dx[s3 + 1] = np.nan, (np.nan, np.nan)      # a dead entry's pose is never looked at
    ref = ml_ref.weighted_averages(Y, img, theta, dx, w, seg, t, chunk)
    assert ref['counts'].tolist() == [sizes[0], 1, 0, 34] and len(set(img[:sizes[0]].tolist())) < sizes[0] // 4
    got = run_weighted(Y, img, theta, dx, w, seg, t)
    c = dict(n=n, C=C, t=t, chunk=chunk, Y=Y, img=img, theta=theta, dx=dx, w=w, seg=seg, E=E, ref=ref, avg=got[0], wsum=got[1],
             counts=got[2])
    for v in list(c.values()) + list(ref.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def check_weighted(got, ref, what):
    avg, wsum, counts = got
    assert not (avg == SENT_F).any() and not (wsum == SENT_F).any() and not (counts == SENT_I).any()
    err = np.abs(avg - ref['avg'])
    has = ref['bound'] > 0
    print(f'{what}: worst error {err.max():.3e}, worst error / bound {(err[has] / ref["bound"][has]).max() if has.any() else 0.0:.3f}')
    assert (err <= ref['bound']).all() and np.isfinite(avg).all()
    assert counts.tolist() == ref['counts'].tolist()
    Ek = np.diff(ref['seg'])
    assert (np.abs(wsum - ref['wsum']) <= Ek * 2.0 ** -53 * ref['wsum']).all()
    for k in np.flatnonzero(ref['wsum'] == 0):
        assert not avg[k].any() and wsum[k] == 0


@pytest.mark.parametrize('n,C', WAVG_GEOMETRIES)
def test_weighted_average_against_fp64(n, C):
    c = wavg_case(n, C)
    check_weighted((c['avg'], c['wsum'], c['counts']), c['ref'], f'weighted average n={n} C={C} t={c["t"]}')
    assert not c['avg'][2].any() and c['wsum'][2] == 0 and c['counts'][2] == 0          # the empty class
    # the class of one: align_stack's image at that pose, to the per-image bound
    e = int(c['seg'][1])
    one = align_ref.align_stack(c['Y'][c['img'][e]][None], c['theta'][e:e + 1], c['dx'][e:e + 1], float(F32(c['t'])))[0]
    assert c['ref']['b'][e] > 0 and np.abs(c['avg'][1] - one).max() <= c['ref']['b'][e]
    assert c['wsum'][1] == 0.75 and c['counts'][1] == 1


@pytest.mark.parametrize('n,C', [(5, 1), (17, 2)])
def test_weighted_average_of_one_entry_is_the_aligned_image_of_the_kernel(n, C):
    """fma(w, a, 0) / w in fp64, rounded once: within an fp32 rounding or two of what tvae_align_stack writes at that pose."""
    from tvae import _cluster_lib as CL
    c = wavg_case(n, C)
    e = int(c['seg'][1])
    i = int(c['img'][e])
    out = torch.full((1, C, n, n), SENT_F, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_align_stack', _dev(c['Y'][i][None]), _dev(c['theta'][e:e + 1]), _dev(c['dx'][e:e + 1]), out, 1, C, n, c['t'])
    a = out.cpu().numpy()[0].astype(np.float64)
    assert (np.abs(c['avg'][1] - a) <= 2 * EPS * np.abs(a)).all()


def test_weighted_average_of_dead_entries_only_is_zero():
    c = wavg_case(5, 1)
    E = 9
    img = np.array([-1, WAVG_N, 3, 4, 5, 6, -(1 << 31), (1 << 31) - 1, 2])
    w = np.array([1.0, 1.0, 0.0, -2.0, np.nan, np.inf, 1.0, 1.0, -np.inf], dtype=F32)
    avg, wsum, counts = run_weighted(c['Y'], img, c['theta'][:E], c['dx'][:E], w, np.array([0, 0, E]), c['t'])
    assert not avg.any() and not wsum.any() and not counts.any() and np.isfinite(avg).all()
    # and beside a live class
    img2, w2 = np.concatenate([img, [7]]), np.concatenate([w, [F32(0.5)]])
    avg, wsum, counts = run_weighted(c['Y'], img2, c['theta'][:E + 1], c['dx'][:E + 1], w2, np.array([0, E, E + 1]), c['t'])
    assert not avg[0].any() and wsum.tolist() == [0.0, 0.5] and counts.tolist() == [0, 1] and avg[1].any()


def test_hostile_seg_is_clamped_on_the_device():
    c = wavg_case(17, 1)
    E = c['E']
    seg = np.array([-7, 120, 100, -5, E + 1000])
    clean = np.array([0, 120, 120, 120, E])
    got = run_weighted(c['Y'], c['img'], c['theta'], c['dx'], c['w'], seg, c['t'])
    want = run_weighted(c['Y'], c['img'], c['theta'], c['dx'], c['w'], clean, c['t'])
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    ref = ml_ref.weighted_averages(c['Y'], c['img'], c['theta'], c['dx'], c['w'], seg, c['t'], c['chunk'])
    assert ref['seg'].tolist() == clean.tolist()
    check_weighted(got, ref, 'hostile seg')


def test_a_class_does_not_depend_on_the_others_or_on_K():
    c = wavg_case(17, 2)
    seg = c['seg']
    s0 = slice(int(seg[0]), int(seg[1]))
    alone = run_weighted(c['Y'], c['img'][s0], c['theta'][s0], c['dx'][s0], c['w'][s0], np.array([0, seg[1]]), c['t'])
    assert alone[0][0].tobytes() == c['avg'][0].tobytes() and alone[1][0] == c['wsum'][0] and alone[2][0] == c['counts'][0]
    s3 = slice(int(seg[3]), int(seg[4]))
    m = int(seg[4] - seg[3])
    moved = run_weighted(c['Y'], c['img'][s3], c['theta'][s3], c['dx'][s3], c['w'][s3], np.array([0, 0, m, m, m, m]), c['t'])
    assert moved[0][1].tobytes() == c['avg'][3].tobytes() and moved[1][1] == c['wsum'][3] and moved[2][1] == c['counts'][3]
    assert not moved[0][[0, 2, 3, 4]].any() and not moved[2][[0, 2, 3, 4]].any()
    # class 3 in front of class 0: other slots, the same bits
    order = np.concatenate([np.arange(seg[3], seg[4]), np.arange(seg[0], seg[1])])
    sw = run_weighted(c['Y'], c['img'][order], c['theta'][order], c['dx'][order], c['w'][order], np.array([0, m, m + seg[1]]), c['t'])
    assert sw[0][0].tobytes() == c['avg'][3].tobytes() and sw[0][1].tobytes() == c['avg'][0].tobytes()
    assert sw[1].tolist() == [c['wsum'][3], c['wsum'][0]]


def test_weighted_average_rejects_unsupported_arguments_and_writes_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    N, C, n, K, E = 4, 1, 8, 2, 6
    Y = torch.zeros(N, C, n, n, device=DEV)
    img = torch.zeros(E, dtype=torch.int32, device=DEV)
    th, dx, w = torch.zeros(E, device=DEV), torch.zeros(E, 2, device=DEV), torch.ones(E, device=DEV)
    seg = torch.tensor([0, 3, 6], dtype=torch.int32, device=DEV)
    avg = torch.full((K, C, n, n), SENT_F, device=DEV)
    wsum = torch.full((K + 1,), SENT_F, dtype=torch.float64, device=DEV)
    counts = torch.full((K,), SENT_I, dtype=torch.int32, device=DEV)
    wsf = CL.query('tvae_class_average_weighted_ws_floats', E, K, C, n)
    ws = CL.workspace(wsf + 2, DEV)
    ws.fill_(SENT_F)
    good = dict(N=N, E=E, C=C, n=n, K=K, wsf=wsf)
    for over in [dict(N=0), dict(N=(1 << 24) + 1), dict(E=0), dict(E=-3), dict(C=0), dict(C=1025), dict(n=1), dict(n=1025), dict(K=0),
                 dict(K=65536), dict(wsf=wsf - 1)]:
        a = dict(good, **over)
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():                   # a rejected call must leave every tensor as it was
                CL.call('tvae_class_average_weighted', Y, img, th, dx, w, seg, avg, wsum[:K], counts, ws[:wsf], a['wsf'], a['N'],
                        a['E'], a['C'], a['n'], a['K'], 1.0)
    with pytest.raises(TvaeHipError):                         # a workspace that starts on an odd word
        with guardband.GuardedCalls():
            CL.call('tvae_class_average_weighted', Y, img, th, dx, w, seg, avg, wsum[:K], counts, ws[1:wsf + 1], wsf, N, E, C, n, K, 1.0)
    with pytest.raises(TvaeHipError):                         # avg over Y
        with guardband.GuardedCalls():
            CL.call('tvae_class_average_weighted', Y, img, th, dx, w, seg, Y[:K], wsum[:K], counts, ws[:wsf], wsf, N, E, C, n, K, 1.0)
    assert (avg == SENT_F).all() and (wsum == SENT_F).all() and (counts == SENT_I).all() and (ws == SENT_F).all()
    assert not Y.any()


def test_python_wrappers_are_bitwise_the_c_abi():
    from tvae import ml2d
    c = wavg_case(17, 2)
    ent = dict(img=_dev(c['img'], torch.int32), theta=_dev(c['theta']), dx=_dev(c['dx']), w=_dev(c['w']), seg=_dev(c['seg'], torch.int32))
    with guardband.GuardedCalls(replay=True):
        avg, wsum, counts = ml2d.weighted_class_averages(_dev(c['Y']), ent, WAVG_K, c['t'])
    assert avg.cpu().numpy().tobytes() == c['avg'].tobytes() and wsum.cpu().numpy().tobytes() == c['wsum'].tobytes()
    assert counts.tolist() == c['counts'].tolist() and wsum.dtype == torch.float64 and counts.dtype == torch.int32
    none = {k: v[:0].contiguous() for k, v in ent.items() if k != 'seg'}
    none['seg'] = torch.zeros(WAVG_K + 1, dtype=torch.int32, device=DEV)
    avg0, wsum0, counts0 = ml2d.weighted_class_averages(_dev(c['Y']), none, WAVG_K, c['t'])
    assert not avg0.any() and not wsum0.any() and not counts0.any()
    p = post_case((5, 4, 2, 8))
    M, A, S, P = p['shape']
    with guardband.GuardedCalls(replay=True):
        post = ml2d.pose_posteriors(_dev(p['num']), _dev(p['pp']), _dev(p['yy']), np.array(p['cand']), _dev(p['theta']), _dev(p['dx']), POST_n,
                                    p['K'], POST_S2, np.array(p['lp']), P, POST_T, A, POST_DTH, S)
    for k, v in p['got'].items():
        assert post[k].cpu().numpy().tobytes() == v.tobytes(), k
    # entries_by_class on the device is what it is on the host
    on_dev = ml2d.entries_by_class(post['cls'], post['w'], post['theta'], post['dx'], p['K'])
    on_host = ml2d.entries_by_class(post['cls'].cpu(), post['w'].cpu(), post['theta'].cpu(), post['dx'].cpu(), p['K'])
    assert all(on_dev[k].is_cuda and torch.equal(on_dev[k].cpu(), on_host[k]) for k in on_host)


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
# |GPU - reference| / |reference| of sigma^2 and of the log-likelihood over the two rounds, measured on an MI355X (the
# docstring of test_loop_against_the_reference quotes the run), and what the test asserts: ten times that, never looser than 1e-3
LOOP_MEASURED = dict(sigma2=2.0 ** -24, log_likelihood=7.9e-9)
LOOP_FLOOR = 1e-3


def run_loop(keep):
    from tvae import ml2d
    p = ml_ref.loop_case()
    with guardband.GuardedCalls(replay=True):
        out = ml2d.ml_rounds(_dev(p['Y']), _dev(p['theta']), _dev(p['dx']), p['cls'], p['K'], p['t'], 2, p['A'] * p['dtheta'], p['A'],
                             p['S'], None, 0.0, keep)
    return p, out


@functools.lru_cache(maxsize=None)
def loop_run():
    return run_loop(ml_ref.LOOP['keep'])


def test_loop_weights_and_reproducibility():
    p, (avg, wsum, lab, th, d, hist) = loop_run()
    N, P = p['N'], ml_ref.LOOP['keep']
    post = hist['posterior']
    live = (post['kept'] > 0).cpu().numpy()
    assert live.all()
    sums = post['w'].double().sum(1).cpu().numpy()
    assert (np.abs(sums - 1.0) <= P * 2.0 ** -23).all()
    assert abs(float(wsum.sum()) - live.sum()) <= N * 2.0 ** -22
    assert np.isfinite(avg.cpu().numpy()).all() and tuple(avg.shape) == (p['K'], 1, p['n'], p['n'])
    assert hist['log_likelihood'].shape == (2,) and hist['sigma2'].shape == (2,) and hist['pi'].shape == (2, p['K'])
    assert tuple(hist['entropy'].shape) == (N,) and bool((hist['entropy'] >= 0).all()) and lab.dtype == torch.int64
    assert torch.equal(th, post['theta'][:, 0]) and torch.equal(d, post['dx'][:, 0])
    resp, cand = post['resp'].cpu().numpy(), hist['candidates'].cpu().numpy()
    assert np.array_equal(lab.cpu().numpy(), cand[np.arange(N), resp.argmax(1)])
    _, again = run_loop(P)
    for a, b in zip((avg, wsum, lab, th, d), again[:5]):
        assert torch.equal(a, b)
    assert np.array_equal(hist['log_likelihood'], again[5]['log_likelihood']) and np.array_equal(hist['sigma2'], again[5]['sigma2'])


def test_loop_in_slices_is_bitwise_the_loop_in_one(monkeypatch):
    """The E-step goes through the stack in slices that bound its tables (tvae.refine.WS_FLOATS): with room for 7 images per
    slice, four slices joined, every result is what the single slice gives, bit for bit."""
    from tvae import ml2d, refine
    p, (avg, wsum, lab, th, d, hist) = loop_run()
    M = p['K']
    per = 2 * M * (2 * p['A'] + 1) * (2 * p['S'] + 1) ** 2 + 1
    assert ml2d._slices(p['N'], M, p['A'], p['S']) == p['N']
    monkeypatch.setattr(refine, 'WS_FLOATS', 7 * per)
    assert ml2d._slices(p['N'], M, p['A'], p['S']) == 7
    _, again = run_loop(ml_ref.LOOP['keep'])
    for a, b in zip((avg, wsum, lab, th, d), again[:5]):
        assert torch.equal(a, b)
    for key in ('idx', 'cls', 'theta', 'dx', 'w', 'resp', 'lse', 'r2', 'kept'):
        assert torch.equal(hist['posterior'][key], again[5]['posterior'][key]), key
    assert np.array_equal(hist['log_likelihood'], again[5]['log_likelihood']) and np.array_equal(hist['sigma2'], again[5]['sigma2'])


def test_loop_with_one_entry_per_image_is_the_hard_average():
    """keep = 1: every weight is exactly 1, and the averages are the plain form of test_align_gpu.py -- the per-class mean of
    align_stack's output at the top-1 poses -- within cnt 2^-24 mean |A| per pixel."""
    from tvae import align
    p, (avg, wsum, lab, th, d, hist) = run_loop(1)
    post = hist['posterior']
    assert bool((post['w'] == 1.0).all()) and bool((post['kept'] > 0).all())
    cls = post['cls'][:, 0].to(torch.int64)
    K = p['K']
    assert np.array_equal(wsum.cpu().numpy(), np.bincount(cls.cpu().numpy(), minlength=K).astype(np.float64))
    with guardband.GuardedCalls(replay=True):
        A = align.align_stack(_dev(p['Y']), th, d, p['t']).cpu().numpy().astype(np.float64)
        hard, cnt = align.class_averages(_dev(p['Y']), th, d, cls, K, p['t'])
    got, c = avg.cpu().numpy(), cls.cpu().numpy()
    for k in range(K):
        m = np.flatnonzero(c == k)
        if m.size == 0:
            assert not got[k].any()
            continue
        tol = m.size * EPS * np.abs(A[m]).mean(0)
        assert (np.abs(got[k] - A[m].mean(0)) <= tol).all() and (np.abs(hard.cpu().numpy()[k] - A[m].mean(0)) <= tol).all(), k
    assert cnt.tolist() == np.bincount(c, minlength=K).tolist()


def test_loop_against_the_reference():
    """sigma^2 and the log-likelihood of both rounds against ml_ref.rounds in fp64 (tests/ml_ref.py: LOOP says how the seed was
    chosen; test_ml2d_cpu.py asserts the clear cut of the reference's own top-P sets).
    Measured on an MI355X: sigma^2 1.0002384185791016 and 1.0045355558395386 on both sides, difference 0 -- both round their
    value to fp32 before the next E-step uses it, so a difference is a multiple of 2^-23 relative or nothing; half of that
    resolution, 2^-24, stands in for the measurement.  Log-likelihood -9961.645504872997 and -9933.788129850343 against
    -9961.645567494535 and -9933.78820795151: 6.3e-9 and 7.9e-9 relative (the tables are fp32 sums on the GPU, fp64 in the
    reference).  Asserted: ten times those, 6.0e-7 and 7.9e-8."""
    p, (avg, wsum, lab, th, d, hist) = loop_run()
    _, ref = ml_ref.loop_reference()
    assert (ref['gaps'] >= 1e-6).all()
    for key in ('sigma2', 'log_likelihood'):
        rel = np.abs(hist[key] - ref[key]) / np.abs(ref[key])
        print(f'ml_rounds {key}: GPU {hist[key].tolist()} reference {ref[key].tolist()} relative difference {rel.tolist()}')
        bound = min(10 * LOOP_MEASURED[key], LOOP_FLOOR)
        assert (rel <= bound).all(), key
    # the same entries in the last round (as sets: two kept candidates of nearly one weight may swap ranks)
    assert np.array_equal(np.sort(hist['posterior']['idx'].cpu().numpy(), 1), np.sort(ref['post']['idx'], 1))
    assert np.array_equal(lab.cpu().numpy(), ref['labels'])
    assert (np.abs(wsum.cpu().numpy() - ref['wsum']) <= 1e-3 * p['N']).all()


def test_loop_with_cross_halves():
    """Every image is scored against the half-set averages it is not in and fills the half it is in: the weights still sum to
    the images, the averages of the whole classes are finite, and two runs are bit-equal."""
    from tvae import ml2d
    p = ml_ref.loop_case()
    runs = []
    for _ in range(2):
        with guardband.GuardedCalls(replay=True):
            runs.append(ml2d.ml_rounds(_dev(p['Y']), _dev(p['theta']), _dev(p['dx']), p['cls'], p['K'], p['t'], 2, p['A'] * p['dtheta'],
                                       p['A'], p['S'], None, 0.0, 4, cross_halves=True))
    avg, wsum, lab, th, d, hist = runs[0]
    N, K = p['N'], p['K']
    assert tuple(avg.shape) == (K, 1, p['n'], p['n']) and np.isfinite(avg.cpu().numpy()).all() and tuple(wsum.shape) == (K,)
    assert bool((hist['posterior']['kept'] > 0).all()) and abs(float(wsum.sum()) - N) <= N * 2.0 ** -22
    cls = hist['posterior']['cls'].cpu().numpy()
    assert ((cls >= -1) & (cls < 2 * K)).all() and np.isfinite(hist['log_likelihood']).all() and (hist['sigma2'] > 0).all()
    assert ((lab >= 0) & (lab < K)).all()
    for a, b in zip(runs[0][:5], runs[1][:5]):
        assert torch.equal(a, b)


def test_ml_class_averages_py_writes_its_files_and_class_averages_py_takes_them(tmp_path):
    p = pose_ref.planted(seed=31, N=6, n=16, K=2)
    rng = np.random.default_rng(32)
    np.save(tmp_path / 'stack.npy', (p['Y'][:, 0] + 0.2 * rng.standard_normal(p['Y'][:, 0].shape)).astype(np.float32))
    np.save(tmp_path / 'rotations.npy', (p['theta_true'] + rng.uniform(-0.1, 0.1, 6)).astype(np.float32).reshape(6, 1))
    np.save(tmp_path / 'translations.npy', (p['dx_true'] + rng.uniform(-0.1, 0.1, (6, 2))).astype(np.float32))
    np.save(tmp_path / 'clusters.npy', p['cls'])
    np.save(tmp_path / 'latents.npy', rng.standard_normal((6, 2)).astype(np.float32))
    stack = ['--stack', str(tmp_path / 'stack.npy'), '--n-clusters', '2']
    cmd = [sys.executable, os.path.join(PKG, 'ml_class_averages.py'), *stack, '--clusters', str(tmp_path / 'clusters.npy'),
           '--rotations', str(tmp_path / 'rotations.npy'), '--translations', str(tmp_path / 'translations.npy'),
           '--latents', str(tmp_path / 'latents.npy'), '--candidates', '2', '--out-dir', str(tmp_path / 'out'), '--rounds', '2',
           '--angle-steps', '4', '--shift', '1', '--keep', '4']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / 'out'
    want = ['class_averages_ml.npy', 'class_weights.npy', 'clusters_ml.npy', 'ml_entropy.npy', 'ml_log_likelihood.npy', 'ml_sigma2.npy',
            'rotations_ml.npy', 'translations_ml.npy']
    assert sorted(os.listdir(out)) in (want, sorted(want + ['class_averages_ml.jpg']))
    lines = [ln for ln in r.stdout.splitlines() if not ln.startswith('#')]
    assert len(lines) == 2 and all(ln.count('->') == 3 for ln in lines)  # one line per class: members and both resolutions
    assert 'log-likelihood' in r.stderr
    lab, rot, tr = np.load(out / 'clusters_ml.npy'), np.load(out / 'rotations_ml.npy'), np.load(out / 'translations_ml.npy')
    assert lab.shape == (6,) and lab.dtype == np.int64 and ((lab >= 0) & (lab < 2)).all()
    assert rot.shape == (6, 1) and rot.dtype == np.float32 and tr.shape == (6, 2) and tr.dtype == np.float32
    w, ll, s2, ent = (np.load(out / f) for f in ('class_weights.npy', 'ml_log_likelihood.npy', 'ml_sigma2.npy', 'ml_entropy.npy'))
    assert w.shape == (2,) and w.dtype == np.float64 and abs(w.sum() - 6) <= 6 * 2.0 ** -22
    assert ll.shape == (2,) and np.isfinite(ll).all() and s2.shape == (2,) and (s2 > 0).all() and ent.shape == (6,) and (ent >= 0).all()
    avg = np.load(out / 'class_averages_ml.npy')
    assert avg.shape == (2, 1, 16, 16) and avg.dtype == np.float32 and np.isfinite(avg).all()
    # the label and pose files go straight into class_averages.py
    cmd = [sys.executable, os.path.join(PKG, 'class_averages.py'), *stack, '--clusters', str(out / 'clusters_ml.npy'),
           '--rotations', str(out / 'rotations_ml.npy'), '--translations', str(out / 'translations_ml.npy'),
           '--out-dir', str(tmp_path / 'again')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    hard = np.load(tmp_path / 'again' / 'class_averages.npy')
    assert hard.shape == avg.shape and np.isfinite(hard).all()


def test_clustering_particles_writes_the_ml_files_and_ml_class_averages_py_reproduces_them(tmp_path):
    """clustering_particles.py on tests/golden/stack_ref.mrcs (5 images cropped to 6 x 6, MLP encoder, t = 0.1) with
    TVAE_ML_AVERAGES=1 adds the maximum-likelihood files beside what it writes anyway, and ml_class_averages.py on the files of
    that run, with its latents and the driver's m = min(K, 8), gives the same files bit for bit."""
    import src.models as M
    torch.manual_seed(2)
    enc = M.InferenceNetwork_UnimodalTranslation_UnimodalRotation(36, 2 + 3, 16, num_layers=2)
    torch.save(enc, tmp_path / 'inference.sav')
    stack = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stack_ref.mrcs')
    cmd = [sys.executable, os.path.join(PKG, 'clustering_particles.py'), '--test-path', stack, '--crop', '6', '--t-inf', 'unimodal',
           '--r-inf', 'unimodal', '--n-clusters', '2', '--path-to-encoder', str(tmp_path / 'inference.sav'), '--out-dir',
           str(tmp_path / 'run')]
    env = {k: v for k, v in os.environ.items() if k not in ('TVAE_CLASS_AVERAGES', 'TVAE_CLASS_FRC', 'TVAE_CLASS_EIGEN', 'TVAE_FIGURES',
                                                            'TVAE_REFINE_POSES', 'TVAE_RECLASSIFY')}
    env['TVAE_ML_AVERAGES'] = '1'
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'maximum-likelihood class averages' in r.stderr
    run = tmp_path / 'run'
    today = ['clusters.npy', 'latents.npy', 'results.txt', 'rotations.npy', 'translations.npy']
    new = ['class_averages_ml.mrcs', 'class_averages_ml.npy', 'class_weights.npy', 'clusters_ml.npy', 'ml_entropy.npy',
           'ml_log_likelihood.npy', 'ml_sigma2.npy', 'rotations_ml.npy', 'translations_ml.npy']
    assert sorted(os.listdir(run)) in (sorted(today + new), sorted(today + new + ['class_averages_ml.jpg']))
    assert np.load(run / 'rotations_ml.npy').shape == np.load(run / 'rotations.npy').shape
    assert abs(np.load(run / 'class_weights.npy').sum() - 5) <= 5 * 2.0 ** -22
    cmd = [sys.executable, os.path.join(PKG, 'ml_class_averages.py'), '--stack', stack, '--crop', '6', '--t-inf', 'unimodal',
           '--n-clusters', '2', '--clusters', str(run / 'clusters.npy'), '--rotations', str(run / 'rotations.npy'), '--translations',
           str(run / 'translations.npy'), '--latents', str(run / 'latents.npy'), '--candidates', '2', '--out-dir', str(tmp_path / 'cli')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    for f in new:
        if f.endswith('.npy'):
            a, b = np.load(run / f), np.load(tmp_path / 'cli' / f)
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), f
    assert open(run / 'class_averages_ml.mrcs', 'rb').read() == open(tmp_path / 'cli' / 'class_averages_ml.mrcs', 'rb').read()
