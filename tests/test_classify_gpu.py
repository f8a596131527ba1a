"""Reassignment against the class averages on the GPU: tvae_pose_classify behind its C ABI (every call under guard bands with
replay, outputs and workspace filled with a sentinel) against the composition it replaces -- M calls of tvae_pose_refine with
cls = cand[:, m], which test_refine_gpu.py pins against fp64, and the rule across slots of tests/classify_ref.py -- then
against fp64 within the bounds of test_refine_gpu.table_bounds (no new tolerance), tvae.classify and reclassify_particles.py.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classify_ref
import guardband
import pose_ref
import test_classify_cpu as TC
import test_refine_gpu as TR
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SENT_F, SENT_I = TR.SENT_F, TR.SENT_I
N_IMG, K_CLS = TR.N_IMG, TR.K_CLS
# (n, C, A, S, N, M): the geometries of test_refine_gpu.py with M at its limit, odd and small
GEOMETRIES = [(8, 1, 1, 1, N_IMG, 64), (17, 2, 2, 3, N_IMG, 3), (32, 3, 8, 2, N_IMG, 4), (33, 1, 0, 8, N_IMG, 2),
              (64, 1, 32, 0, N_IMG, 2), (128, 1, 2, 3, 3, 2)]
CASES = [g + (m,) for g in GEOMETRIES for m in (False, True)]
NAMES = ('cls', 'best', 'theta', 'dx', 'score', 'num', 'pp', 'yy')


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def run_classify(Y, theta, dx, cand, refs, A, S, t, dtheta, radius=0.0, edge=0.0, tables=True):
    """tvae_pose_classify into sentinel-filled outputs and workspace -> dict of numpy arrays."""
    from tvae import _cluster_lib as CL
    N, C, n, _ = Y.shape
    M = np.asarray(cand).shape[1]
    K, NA, NS = refs.shape[0], 2 * A + 1, 2 * S + 1
    wsf = CL.query('tvae_pose_classify_ws_floats', N, M, C, n, A, S)
    assert wsf == N * (2 * M * NA * NS * NS + 1)
    ws = torch.full((wsf,), SENT_F, device=DEV)
    th_out, dx_out, score = (torch.full(s, SENT_F, device=DEV) for s in ((N,), (N, 2), (N, M, 2)))
    cls_out = torch.full((N,), SENT_I, dtype=torch.int32, device=DEV)
    best = torch.full((N, 4), SENT_I, dtype=torch.int32, device=DEV)
    num = pp = yy = None
    if tables:
        num, pp, yy = (torch.full(s, SENT_F, device=DEV) for s in ((N, M, NA, NS, NS), (N, M, NA, NS, NS), (N,)))
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_classify', _dev(Y), _dev(theta), _dev(dx), _dev(cand, torch.int32), _dev(refs), cls_out, best, th_out,
                dx_out, score, num, pp, yy, ws, wsf, N, C, n, K, M, A, S, t, dtheta, radius, edge)
    out = dict(cls=cls_out, best=best, theta=th_out, dx=dx_out, score=score, num=num, pp=pp, yy=yy)
    out = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    for k, v in out.items():
        assert not (v == (SENT_I if k in ('cls', 'best') else SENT_F)).any(), k
    return out


def make_candidates(cls, M, seed):
    """Slot 0 the labels of test_refine_gpu.make_inputs (a -1 and a 7 among them), the other slots drawn from the classes, -1 and
    values >= K; a duplicate, a row of one class throughout and a row with no valid slot are planted."""
    rng = np.random.default_rng(seed)
    N = cls.size
    cand = rng.choice([0, 1, 2, 3, 0, 1, 3, -1, K_CLS, 9], (N, M))
    cand[:, 0] = cls
    if M > 1:
        cand[0, 1] = cand[0, 0]                               # a duplicate of slot 0
        cand[1, :] = 3                                        # one class in every slot
        cand[2, 0], cand[2, 1] = -1, 1                        # slot 0 skipped, slot 1 valid
    last = N - 1 if N < N_IMG else 5
    cand[last, :] = rng.choice([-1, K_CLS, 1 << 20, -(1 << 30)], M)      # no valid slot (image 5 of the full set has cls = -1)
    return cand.astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(n, C, A, S, N, M, masked):
    """Inputs, the guarded GPU results of tvae_pose_classify and of the M calls of tvae_pose_refine it must reproduce."""
    t = 1.0 if n in (8, 32, 64) else 0.1
    dtheta = 0.02 if A > 8 else 0.05
    radius, edge = (0.3 * n, max(2.0, 0.15 * n)) if masked else (0.0, 0.0)
    Y, refs, theta, dx, cls = TR.make_inputs(n, C, N, 100 * n + C)
    dx = (dx / np.float32(t)).astype(np.float32)
    cand = make_candidates(cls, M, 7 * n + M)
    got = run_classify(Y, theta, dx, cand, refs, A, S, t, dtheta, radius, edge)
    slots = [TR.run_refine(Y, theta, dx, cand[:, m], refs, A, S, t, dtheta, radius, edge) for m in range(M)]
    c = dict(n=n, C=C, A=A, S=S, N=N, M=M, t=t, dtheta=dtheta, radius=radius, edge=edge, Y=Y, refs=refs, theta=theta, dx=dx,
             cand=cand, got=got, slots=slots)
    for d in [c, got] + slots:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c


# ---- 1. bitwise against the composition --------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C,A,S,N,M,masked', CASES)
def test_every_slot_is_pose_refine_bit_for_bit_and_the_winner_follows_the_rule(n, C, A, S, N, M, masked):
    c = case(n, C, A, S, N, M, masked)
    got, slots, cand = c['got'], c['slots'], c['cand']
    valid = (cand >= 0) & (cand < K_CLS)
    assert valid.any(1).sum() >= 2 and (~valid.any(1)).any() and (~valid).any()
    for m in range(M):
        for nm in ('num', 'pp'):
            assert np.array_equal(bits(got[nm][:, m]), bits(slots[m][nm])), (nm, m)
        assert np.array_equal(bits(got['score'][:, m]), bits(slots[m]['score'])), m
        ok = valid[:, m]
        assert np.array_equal(bits(got['yy'][ok]), bits(slots[m]['yy'][ok])), m      # one sum per image, the sum of every slot
        assert not got['num'][~ok, m].any() and not got['pp'][~ok, m].any() and not got['score'][~ok, m].any()
    assert not got['yy'][~valid.any(1)].any()
    slot_out = np.stack([s['score'] for s in slots], 1)
    slot_best = np.stack([s['best'] for s in slots], 1)
    cls_out, best = classify_ref.choose(slot_out, slot_best, cand, K_CLS)
    th, d = pose_ref.update_pose(c['theta'], c['dx'], best[:, 1:], n, c['t'], c['dtheta'])
    assert np.array_equal(got['cls'], np.clip(cls_out, -(1 << 31), (1 << 31) - 1)) and np.array_equal(got['best'], best)
    assert np.array_equal(bits(got['theta']), bits(th)) and np.array_equal(bits(got['dx']), bits(d))
    w = best[:, 0]
    for i in range(N):                                        # the winner's pose is that slot's refined pose
        if valid[i].any():
            assert bits(got['theta'])[i] == bits(slots[w[i]]['theta'])[i] and np.array_equal(bits(got['dx'])[i], bits(slots[w[i]]['dx'])[i])
            assert (got['score'][i, w[i], 1] >= got['score'][i, valid[i], 1]).all()
    none = ~valid.any(1)
    assert np.array_equal(bits(got['theta'][none]), bits(c['theta'][none])) and np.array_equal(bits(got['dx'][none]), bits(c['dx'][none]))
    assert not got['best'][none].any() and np.array_equal(got['cls'][none], cand[none, 0].astype(np.int32))
    if M > 1 and N == N_IMG:
        assert got['best'][0, 0] != 1 and got['best'][1, 0] == 0 and got['best'][2, 0] >= 1      # duplicates never win; slot 0 skipped


@pytest.mark.parametrize('masked', [False, True])
def test_one_candidate_is_pose_refine_in_every_output(masked):
    c = case(17, 2, 2, 3, N_IMG, 3, masked)
    cls = c['cand'][:, :1]
    got = run_classify(c['Y'], c['theta'], c['dx'], cls, c['refs'], 2, 3, c['t'], c['dtheta'], c['radius'], c['edge'])
    one = c['slots'][0]
    for nm, mine in (('theta', got['theta']), ('dx', got['dx']), ('score', got['score'][:, 0]), ('best', got['best'][:, 1:]),
                     ('num', got['num'][:, 0]), ('pp', got['pp'][:, 0]), ('yy', got['yy'])):
        assert np.array_equal(bits(mine), bits(one[nm])), nm
    assert np.array_equal(got['cls'], cls[:, 0].astype(np.int32)) and not got['best'][:, 0].any()


# ---- 2. against fp64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C,A,S,N,M,masked', [(17, 2, 2, 3, N_IMG, 3, True), (32, 3, 8, 2, N_IMG, 4, False)])
def test_tables_against_fp64(n, C, A, S, N, M, masked):
    c = case(n, C, A, S, N, M, masked)
    got = c['got']
    t64 = float(np.float32(c['t']))
    for m in range(M):
        cls = c['cand'][:, m]
        ref = pose_ref.refine(c['Y'], c['theta'], c['dx'], cls, c['refs'], t64, A, c['dtheta'], S, c['radius'] if masked else None,
                              c['edge'])
        bnd = TR.table_bounds(dict(c, cls=cls, ref=ref))
        ok = (cls >= 0) & (cls < K_CLS)
        for nm, mine in (('num', got['num'][:, m]), ('pp', got['pp'][:, m]), ('yy', np.where(ok, got['yy'], 0.0))):
            err = np.abs(mine - ref[nm])
            live = bnd[nm] > 0
            worst = (err[live] / bnd[nm][live]).max() if live.any() else 0.0
            print(f'pose_classify n={n} slot {m} mask={masked} {nm}: worst error {err.max():.3e}, worst error / bound {worst:.3f}')
            assert (err <= bnd[nm]).all(), (nm, m, np.argwhere(err > bnd[nm])[:5])
        dead = bnd['dead']
        assert not got['num'][dead, m].any() and not got['pp'][dead, m].any()


# ---- 3. recovery -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(seed=7), dict(seed=41, N=24, K=4, n=17, A=2, S=3)])
def test_planted_classes_and_poses_are_recovered(kw):
    p = pose_ref.planted(**kw)
    start = TC.mislabel(p)
    assert (start[::3] != p['cls'][::3]).all()
    cand = classify_ref.candidate_lists(start, p['K'])
    got = run_classify(p['Y'], p['theta'], p['dx'], cand, p['refs'], p['A'], p['S'], p['t'], p['dtheta'])
    assert np.array_equal(got['cls'], p['cls']), np.flatnonzero(got['cls'] != p['cls'])
    assert np.array_equal(got['best'][:, 1:], p['want']), np.flatnonzero((got['best'][:, 1:] != p['want']).any(1))
    win = got['score'][np.arange(p['N']), got['best'][:, 0], 1]
    assert (win > 1 - 1e-4).all() and (got['best'][::3, 0] > 0).all()


# ---- 4. ties and skipping --------------------------------------------------------------------------------------------------------
def test_ties_stay_with_slot_0_and_skipped_references_are_never_read():
    c = case(32, 3, 8, 2, N_IMG, 4, False)
    args = (c['A'], c['S'], c['t'], c['dtheta'])
    N = N_IMG
    refs = c['refs'].copy()
    refs[1] = refs[0]                                         # two classes with one reference, bit for bit
    rows = np.array([[1, 0], [0, 1], [3, 3]] * (N // 3))
    got = run_classify(c['Y'], c['theta'], c['dx'], rows, refs, *args)
    assert not got['best'][:, 0].any() and np.array_equal(got['cls'], rows[:, 0].astype(np.int32))
    assert np.array_equal(bits(got['score'][:, 0]), bits(got['score'][:, 1]))
    # a NaN reference in a class that no row names changes no bit
    refs2 = refs.copy()
    refs2[2] = np.nan
    other = run_classify(c['Y'], c['theta'], c['dx'], rows, refs2, *args)
    for k in got:
        assert np.array_equal(bits(other[k]), bits(got[k])), k
    # every reference NaN: a row with no valid slot reads nothing of them, and a skipped slot costs zeros
    nan = run_classify(c['Y'], c['theta'], c['dx'], c['cand'], np.full_like(c['refs'], np.nan), *args)
    valid = (c['cand'] >= 0) & (c['cand'] < K_CLS)
    none = ~valid.any(1)
    for k in NAMES:
        assert np.array_equal(bits(nan[k][none]), bits(c['got'][k][none])), k
    assert not nan['num'][~valid].any() and not nan['pp'][~valid].any() and not nan['score'][~valid].any()
    # rows that name class 0 alone, between skipped slots: NaN in every other reference leaves their bits alone
    refs3 = np.full_like(c['refs'], np.nan)
    refs3[0] = c['refs'][0]
    rows = np.array([[-1, 0, K_CLS, 0]] * N)
    a = run_classify(c['Y'], c['theta'], c['dx'], rows, refs3, *args)
    b = run_classify(c['Y'], c['theta'], c['dx'], rows, c['refs'], *args)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert (a['best'][:, 0] == 1).all() and (a['cls'] == 0).all()


# ---- 5. independence and reproducibility -------------------------------------------------------------------------------------------
def test_independent_of_the_other_images_and_of_K_and_reproducible(monkeypatch):
    from tvae import classify, refine
    c = case(17, 2, 2, 3, N_IMG, 3, True)
    got = c['got']
    args = (c['A'], c['S'], c['t'], c['dtheta'], c['radius'], c['edge'])
    again = run_classify(c['Y'], c['theta'], c['dx'], c['cand'], c['refs'], *args)
    for k in got:
        assert np.array_equal(bits(again[k]), bits(got[k])), k
    sub = np.array([19, 3, 4, 9, 16, 0, 22, 5])
    part = run_classify(c['Y'][sub], c['theta'][sub], c['dx'][sub], c['cand'][sub], c['refs'], *args)
    # K doubled with unused references: values that were >= K and are now valid must be moved out of the way
    cand2 = np.where((c['cand'] >= K_CLS) & (c['cand'] < 2 * K_CLS), 2 * K_CLS + 1, c['cand'])
    more = run_classify(c['Y'], c['theta'], c['dx'], cand2, np.concatenate([c['refs'], np.ones_like(c['refs'])]), *args, tables=False)
    for k in got:
        assert np.array_equal(bits(part[k]), bits(got[k][sub])), k
        if k in more and k != 'cls':
            assert np.array_equal(bits(more[k]), bits(got[k])), k
    assert np.array_equal(more['cls'], np.clip(cand2, -(1 << 31), (1 << 31) - 1)[np.arange(N_IMG), got['best'][:, 0]])
    # the Python API is bitwise the C ABI, whole and in slices of the stack

    def api():
        with guardband.GuardedCalls(replay=True):
            return classify.classify_poses(_dev(c['Y']), _dev(c['theta']).view(-1, 1), _dev(c['dx']), c['cand'].copy(),
                                           _dev(c['refs']), c['t'], c['A'], c['dtheta'], c['S'], c['radius'], c['edge'], tables=True)

    whole = api()
    per = 2 * 3 * 5 * 49 + 1                                  # floats of workspace of one image: M = 3, NA = 5, NS = 7
    monkeypatch.setattr(refine, 'WS_FLOATS', 5 * per + 3)      # five images per call
    sliced = api()
    for res in (whole, sliced):
        for v, k in zip(res, ('cls', 'theta', 'dx', 'score', 'best', 'num', 'pp', 'yy')):
            assert np.array_equal(bits(v.cpu().numpy().astype(np.int32) if k == 'cls' else v.cpu().numpy()), bits(got[k])), k
    assert whole[0].dtype == torch.int64 and whole[4].dtype == torch.int32 and tuple(whole[3].shape) == (N_IMG, 3, 2)
    assert len(classify.classify_poses(_dev(c['Y']), _dev(c['theta']), _dev(c['dx']), torch.from_numpy(c['cand'].copy()),
                                       _dev(c['refs']), c['t'], 1, None, 1)) == 5


# ---- 6. rejection ------------------------------------------------------------------------------------------------------------------
def test_unsupported_arguments_are_rejected_and_write_nothing():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    N, C, n, K, M, A, S = 4, 1, 8, 2, 2, 1, 1
    Y, refs = torch.zeros(N, C, n, n, device=DEV), torch.zeros(K, C, n, n, device=DEV)
    th, dx = torch.zeros(N, device=DEV), torch.zeros(N, 2, device=DEV)
    cand = torch.zeros(N, 65, dtype=torch.int32, device=DEV)              # wide enough for M = 65
    wsf = CL.query('tvae_pose_classify_ws_floats', N, M, C, n, A, S)
    big = CL.query('tvae_pose_classify_ws_floats', N, 64, C, n, A, S) * 2  # room for what a wrongly accepted call would write
    outs = [torch.full(s, SENT_F, device=DEV) for s in ((N,), (N, 2), (N, 65, 2))]
    cls_out = torch.full((N,), SENT_I, dtype=torch.int32, device=DEV)
    best = torch.full((N, 4), SENT_I, dtype=torch.int32, device=DEV)
    num, pp = (torch.full((N, 65, 3, 3, 3), SENT_F, device=DEV) for _ in range(2))
    yy, ws = torch.full((N,), SENT_F, device=DEV), torch.full((big,), SENT_F, device=DEV)

    def attempt(N=N, C=C, n=n, K=K, M=M, A=A, S=S, t=1.0, dth=0.1, radius=0.0, edge=0.0, th_out=outs[0], cls_out=cls_out, num=num,
                pp=pp, wsf=big):
        with pytest.raises(TvaeHipError):
            with guardband.GuardedCalls():                               # a rejected call must leave every tensor as it was
                CL.call('tvae_pose_classify', Y, th, dx, cand, refs, cls_out, best, th_out, outs[1], outs[2], num, pp, yy, ws,
                        wsf, N, C, n, K, M, A, S, t, dth, radius, edge)

    for kw in (dict(M=0), dict(M=65), dict(n=129), dict(A=33), dict(S=9), dict(C=17), dict(t=0.0), dict(dth=float('nan')),
               dict(pp=None), dict(num=None), dict(th_out=th), dict(cls_out=cand), dict(wsf=wsf - 1), dict(n=1), dict(N=0),
               dict(K=0), dict(K=65536), dict(A=-1), dict(S=-1), dict(M=-1), dict(t=float('inf')), dict(t=-1.0),
               dict(dth=float('inf')), dict(edge=-1.0), dict(radius=float('nan')), dict(edge=float('inf'))):
        attempt(**kw)
    for t_ in outs + [num, pp, yy, ws]:
        assert (t_ == SENT_F).all()
    assert (best == SENT_I).all() and (cls_out == SENT_I).all() and not cand.any()
    for bad in [(N, 0, C, n, A, S), (N, 65, C, n, A, S), (N, M, C, 129, A, S), (N, M, C, n, 33, S), (N, M, C, n, A, 9), (N, M, 17, n, A, S)]:
        assert CL.query('tvae_pose_classify_ws_floats', *bad) == 0


# ---- 7. classify_rounds end to end -----------------------------------------------------------------------------------------------
def test_classify_rounds_recovers_the_planted_classes():
    from tvae import align, classify
    p, theta0, dx0, labels0 = TC.rounds_start()
    K = p['K']
    Y, th0, d0 = _dev(p['Y']), _dev(theta0), _dev(dx0)
    assert (labels0 != p['cls']).sum() == 20
    with guardband.GuardedCalls(replay=True):
        lab, th, d, hist = classify.classify_rounds(Y, th0, d0, labels0, K, 1.0, rounds=3, angle_range=np.pi / 8, angle_steps=8,
                                                    shift=2)
    sc = hist['scores']
    print('classify_rounds: moved', hist['moved'].tolist(), 'mean incumbent-centre / winning score per round', sc.tolist())
    assert lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), p['cls'])
    assert hist['moved'].shape == (3,) and hist['moved'][-1] == 0 and hist['moved'][0] > 0
    assert hist['counts'].shape == (4, K) and np.array_equal(hist['counts'][0], np.bincount(labels0, minlength=K))
    assert np.array_equal(hist['counts'][-1], np.bincount(p['cls'], minlength=K))
    assert hist['steps'] == [np.pi / 64, np.pi / 128, np.pi / 256]
    assert sc.shape == (3, 2) and sc.dtype == np.float64 and (np.diff(sc[:, 1]) >= 0).all()
    start = align.class_averages(Y, th0, d0, labels0, K, 1.0)[0].cpu().numpy().astype(np.float64)
    final = align.class_averages(Y, th, d, lab, K, 1.0)[0].cpu().numpy().astype(np.float64)
    l2 = lambda a: np.sqrt(((a - p['refs']) ** 2).sum(axis=(1, 2, 3)))
    print('classify_rounds: L2 distance of the class averages from the planted references', l2(start).tolist(), '->', l2(final).tolist())
    assert (l2(final) < l2(start)).all()
    cs = classify.class_scores(hist['candidates'], hist['slot_scores'], K)
    assert cs.shape == (60, K) and cs.dtype == np.float32 and np.array_equal(cs.argmax(1), p['cls'])


def test_cross_halves_never_score_an_image_against_an_average_that_contains_it():
    """One round with cross_halves: an image of half 0 is scored against the half-1 averages of its own and of every other class,
    so altering OTHER images of half 0 leaves its result bit for bit; the images of half 1, whose references those images are
    part of, do change."""
    from tvae import classify
    p, theta0, dx0, _ = TC.rounds_start()
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
            lab, th, d, hist = classify.classify_rounds(_dev(y), _dev(theta0), _dev(dx0), p['cls'], K, 1.0, rounds=1, cross_halves=True)
        res.append((lab.cpu().numpy(), th.cpu().numpy(), d.cpu().numpy(), hist['slot_scores'].cpu().numpy()))
    same = np.setdiff1d(half0, altered)
    assert same.size and ((res[0][0] >= 0) & (res[0][0] < K)).all()
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(bits(a[same]), bits(b[same]))
    assert not all(np.array_equal(a[half1], b[half1]) for a, b in zip(res[0][1:], res[1][1:]))


# ---- 8. the command line -------------------------------------------------------------------------------------------------------
def test_reclassify_particles_py_writes_its_files_and_class_averages_py_reproduces_the_averages(tmp_path):
    p = pose_ref.planted(seed=31, N=6, n=16, K=2)
    rng = np.random.default_rng(32)
    np.save(tmp_path / 'stack.npy', p['Y'][:, 0])
    np.save(tmp_path / 'rotations.npy', (p['theta_true'] + rng.uniform(-0.1, 0.1, 6)).astype(np.float32).reshape(6, 1))
    np.save(tmp_path / 'translations.npy', (p['dx_true'] + rng.uniform(-0.1, 0.1, (6, 2))).astype(np.float32))
    start = p['cls'].copy()
    start[0] = 1 - start[0]
    np.save(tmp_path / 'clusters.npy', start)
    np.save(tmp_path / 'latents.npy', rng.standard_normal((6, 2)).astype(np.float32))
    stack = ['--stack', str(tmp_path / 'stack.npy'), '--n-clusters', '2']
    cmd = [sys.executable, os.path.join(PKG, 'reclassify_particles.py'), *stack, '--clusters', str(tmp_path / 'clusters.npy'),
           '--rotations', str(tmp_path / 'rotations.npy'), '--translations', str(tmp_path / 'translations.npy'),
           '--latents', str(tmp_path / 'latents.npy'), '--candidates', '2', '--out-dir', str(tmp_path / 'out'), '--rounds', '2',
           '--angle-steps', '4', '--shift', '1']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / 'out'
    want = ['class_averages_reclassified.npy', 'class_scores.npy', 'classify_moved.npy', 'classify_scores.npy',
            'clusters_reclassified.npy', 'rotations_reclassified.npy', 'translations_reclassified.npy']
    assert sorted(os.listdir(out)) in (want, sorted(want + ['class_averages_reclassified.jpg']))
    lines = [ln for ln in r.stdout.splitlines() if not ln.startswith('#')]
    assert len(lines) == 2 and all(ln.count('->') == 3 for ln in lines)  # one line per class: members and both resolutions
    lab = np.load(out / 'clusters_reclassified.npy')
    rot, tr = np.load(out / 'rotations_reclassified.npy'), np.load(out / 'translations_reclassified.npy')
    assert lab.shape == (6,) and lab.dtype == np.int64 and ((lab >= 0) & (lab < 2)).all()
    assert rot.shape == (6, 1) and rot.dtype == np.float32 and tr.shape == (6, 2) and tr.dtype == np.float32
    sc, mv, cs = np.load(out / 'classify_scores.npy'), np.load(out / 'classify_moved.npy'), np.load(out / 'class_scores.npy')
    assert sc.shape == (2, 2) and sc.dtype == np.float64 and mv.shape == (2,) and mv.dtype.kind == 'i'
    assert cs.shape == (6, 2) and cs.dtype == np.float32 and np.isfinite(cs).all() and np.array_equal(cs.argmax(1), lab)
    avg = np.load(out / 'class_averages_reclassified.npy')
    assert avg.shape == (2, 1, 16, 16) and avg.dtype == np.float32
    cmd = [sys.executable, os.path.join(PKG, 'class_averages.py'), *stack, '--clusters', str(out / 'clusters_reclassified.npy'),
           '--rotations', str(out / 'rotations_reclassified.npy'), '--translations', str(out / 'translations_reclassified.npy'),
           '--out-dir', str(tmp_path / 'again')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.array_equal(np.load(tmp_path / 'again' / 'class_averages.npy'), avg)


def test_clustering_particles_reclassifies_and_reclassify_particles_py_reproduces_it(tmp_path):
    """clustering_particles.py on tests/golden/stack_ref.mrcs (5 images cropped to 6 x 6, MLP encoder, t = 0.1) with
    TVAE_RECLASSIFY=1 adds the reclassified files beside what it writes anyway, and reclassify_particles.py on the files of that run,
    with its latents and the driver's m = min(K, 8), gives the same labels, poses and averages bit for bit."""
    import src.models as M
    torch.manual_seed(2)
    enc = M.InferenceNetwork_UnimodalTranslation_UnimodalRotation(36, 2 + 3, 16, num_layers=2)
    torch.save(enc, tmp_path / 'inference.sav')
    stack = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stack_ref.mrcs')
    cmd = [sys.executable, os.path.join(PKG, 'clustering_particles.py'), '--test-path', stack, '--crop', '6', '--t-inf', 'unimodal',
           '--r-inf', 'unimodal', '--n-clusters', '2', '--path-to-encoder', str(tmp_path / 'inference.sav'), '--out-dir',
           str(tmp_path / 'run')]
    env = {k: v for k, v in os.environ.items() if k not in ('TVAE_CLASS_AVERAGES', 'TVAE_CLASS_FRC', 'TVAE_FIGURES', 'TVAE_REFINE_POSES')}
    env['TVAE_RECLASSIFY'] = '1'
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'reassigning the images' in r.stderr
    run = tmp_path / 'run'
    today = ['clusters.npy', 'latents.npy', 'results.txt', 'rotations.npy', 'translations.npy']
    new = ['class_averages_reclassified.mrcs', 'class_averages_reclassified.npy', 'class_scores.npy', 'classify_moved.npy',
           'classify_scores.npy', 'clusters_reclassified.npy', 'rotations_reclassified.npy', 'translations_reclassified.npy']
    assert sorted(os.listdir(run)) in (sorted(today + new), sorted(today + new + ['class_averages_reclassified.jpg']))
    assert np.load(run / 'rotations_reclassified.npy').shape == np.load(run / 'rotations.npy').shape
    cmd = [sys.executable, os.path.join(PKG, 'reclassify_particles.py'), '--stack', stack, '--crop', '6', '--t-inf', 'unimodal',
           '--n-clusters', '2', '--clusters', str(run / 'clusters.npy'), '--rotations', str(run / 'rotations.npy'), '--translations',
           str(run / 'translations.npy'), '--latents', str(run / 'latents.npy'), '--candidates', '2', '--out-dir', str(tmp_path / 'cli')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    for f in new:
        if f.endswith('.npy'):
            a, b = np.load(run / f), np.load(tmp_path / 'cli' / f)
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), f
