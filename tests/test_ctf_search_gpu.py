"""The CTF-aware hard search on the GPU: tvae_pose_select behind its C ABI (every call under guard bands with replay, the outputs
filled with a sentinel) against the restatement tests/ctf_search_ref.py, bit for bit -- the kernel's score is three correctly
rounded fp64 operations and one conversion, which numpy restates exactly, and the rest is comparisons and the fp32 pose update
of pose_ref.update_pose; no tolerance anywhere in this file.  Then tvae.ctf.select_poses, classify_poses(ctf=...),
refine_poses(ctf=...) against the hand composition of their parts, and the rounds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ctf_pose_ref as R
import ctf_search_ref as SR
import guardband
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32 = np.float32
SENT_F = -12345.5
SENT_I = -7777777
OUTS = ('cls', 'best', 'theta', 'dx', 'score')


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == F32 else a


def same(got, want, keys=OUTS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(_bits(got[k]), _bits(want[k])), k


def run_select(theta, dx, cand, num, pp, yy, n, K, A, S, t=1.0, dtheta=0.05, **over):
    """tvae_pose_select into sentinel-filled outputs -> dict of numpy arrays.  The tensors have the shapes of the arrays; n, K, A
    and S only go into the call, and `over` replaces its N, M and pp_per_shift."""
    from tvae import _cluster_lib as CL
    cand = np.asarray(cand)
    N, M = cand.shape
    per_shift = int(np.asarray(pp).ndim == 5)
    o = dict(cls=torch.full((N,), SENT_I, dtype=torch.int32, device=DEV), best=torch.full((N, 4), SENT_I, dtype=torch.int32, device=DEV),
             theta=torch.full((N,), SENT_F, device=DEV), dx=torch.full((N, 2), SENT_F, device=DEV),
             score=torch.full((N, M, 2), SENT_F, device=DEV))
    try:
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_pose_select', _dev(theta), _dev(dx), _dev(cand, torch.int32), _dev(num), _dev(pp), _dev(yy), *o.values(),
                    over.get('N', N), over.get('n', n), over.get('K', K), over.get('M', M), over.get('A', A), over.get('S', S),
                    over.get('per_shift', per_shift), float(t), float(dtheta))
    finally:
        run_select.last = {k: v.cpu().numpy() for k, v in o.items()}
    return run_select.last


def untouched(last):
    return all((v == (SENT_I if v.dtype == np.int32 else F32(SENT_F))).all() for v in last.values())


def random_tables(N, M, A, S, K, seed):
    rng = np.random.default_rng(seed)
    NA, NS = 2 * A + 1, 2 * S + 1
    return dict(num=rng.standard_normal((N, M, NA, NS, NS)).astype(F32), ppc=rng.uniform(0.5, 2.0, (N, M, NA)).astype(F32),
                pp=rng.uniform(0.5, 2.0, (N, M, NA, NS, NS)).astype(F32), yy=rng.uniform(0.5, 2.0, N).astype(F32),
                cand=rng.integers(-1, K + 1, (N, M)), theta=rng.uniform(-3, 3, N).astype(F32),
                dx=rng.uniform(-0.2, 0.2, (N, 2)).astype(F32))


# ---- 1. the kernel against the restatement -----------------------------------------------------------------------------------------
# (1, 1, 0, 0) a single candidate; (257, 4, 3, 2) 175 candidates per slot, no multiple of 64, N no multiple of 4; (3, 64, 1, 0) the
# most slots; (2, 2, 32, 8) the corner of the range
@pytest.mark.parametrize('per_shift', [0, 1])
@pytest.mark.parametrize('N,M,A,S', [(1, 1, 0, 0), (5, 3, 2, 1), (257, 4, 3, 2), (3, 64, 1, 0), (2, 2, 32, 8)])
def test_random_tables_bit_for_bit(N, M, A, S, per_shift):
    K, n = 5, 17
    c = random_tables(N, M, A, S, K, 100 * N + M)
    c['cand'][0, 0] = 2                                        # (at least one live slot)
    pp = c['pp'] if per_shift else c['ppc']
    got = run_select(c['theta'], c['dx'], c['cand'], c['num'], pp, c['yy'], n, K, A, S, 1.5, 0.03)
    same(got, SR.select_ref(c['num'], pp, c['yy'], c['cand'], c['theta'], c['dx'], n, K, A, S, 1.5, 0.03))


# ---- 2. the branches, each with a planted table --------------------------------------------------------------------------------------
def test_ties():
    """pp = yy = 1, so a score is its num exactly.  A = 2, S = 2: 125 candidates (two lane passes), the centre is index 62."""
    A, S, K, n, M = 2, 2, 3, 20, 2
    cnd, ci = 125, 62
    num = np.full((6, M, cnd), -1.0, dtype=F32)
    cand = np.array([[0, 1], [0, -1], [0, -1], [0, -1], [1, 1], [0, 2]])
    num[0] = 0.5                                               # all equal: the centre, and the lowest slot
    num[1, 0, [100, 7]] = 0.75                                 # equal maxima off centre: the lowest index
    num[2, 0, [70, 5]] = 0.75                                  # ... on both sides of 64, in different lanes
    num[3, 0, [70, 6]] = 0.75                                  # ... and in one lane's two passes
    num[4, :, 30] = 0.25                                       # duplicate candidates across slots: the lowest slot
    num[5, 0, 9], num[5, 1, 11] = 0.25, 0.5                    # a strictly greater later slot wins
    theta, dx = np.linspace(-1, 1, 6).astype(F32), np.full((6, 2), 0.01, dtype=F32)
    table = num.reshape(6, M, 5, 5, 5)
    got = run_select(theta, dx, cand, table, np.ones_like(table), np.ones(6, dtype=F32), n, K, A, S)
    unflat = lambda e: [e // 25 - A, (e // 5) % 5 - S, e % 5 - S]
    assert got['best'].tolist() == [[0, 0, 0, 0], [0] + unflat(7), [0] + unflat(5), [0] + unflat(6), [0] + unflat(30), [1] + unflat(11)]
    assert got['cls'].tolist() == [0, 0, 0, 0, 1, 2]
    assert got['score'][:, 0].tolist() == [[0.5, 0.5], [-1, 0.75], [-1, 0.75], [-1, 0.75], [-1, 0.25], [-1, 0.25]]
    assert got['score'][:, 1].tolist() == [[0.5, 0.5], [0, 0], [0, 0], [0, 0], [-1, 0.25], [-1, 0.5]]
    assert got['theta'][0].view(np.int32) == theta[0].view(np.int32) and np.array_equal(_bits(got['dx'][0]), _bits(dx[0]))
    same(got, SR.select_ref(table, np.ones_like(table), np.ones(6, dtype=F32), cand, theta, dx, n, K, A, S, 1.0, 0.05))


def test_non_finite_inputs():
    """A = 1, S = 1: 27 candidates, the centre is index 13; the template power per angle."""
    A, S, K, n = 1, 1, 2, 16
    nan, inf = np.nan, np.inf
    num = np.full((6, 1, 27), -0.5, dtype=F32)
    ppc, yy = np.ones((6, 1, 3), dtype=F32), np.ones(6, dtype=F32)
    num[0, 0, :4] = [nan, inf, -inf, 0.25]                     # NaN and +-inf are skipped: index 3 wins
    ppc[1, 0, 0] = 0.0                                         # pp = 0: exact zeros, above the -0.5 elsewhere; the lowest index
    num[2, 0, 18:] = 5.0                                       # negative pp: NaN scores, skipped
    ppc[2, 0, 2] = -1.0
    num[2, 0, 4] = 0.0
    yy[3] = 0.0                                                # yy = 0: every score is 0, the centre wins
    num[4, 0, 13] = nan                                        # the centre is not finite: sc = -inf
    num[4, 0, 20] = 0.125
    num[5] = nan                                               # nothing finite: (0, 0), the centre, the pose as it was
    theta, dx = np.linspace(-1, 1, 6).astype(F32), np.full((6, 2), -0.02, dtype=F32)
    table = num.reshape(6, 1, 3, 3, 3)
    got = run_select(theta, dx, np.zeros((6, 1), dtype=np.int64), table, ppc, yy, n, K, A, S)
    unflat = lambda e: [0, e // 9 - A, (e // 3) % 3 - S, e % 3 - S]
    assert got['best'].tolist() == [unflat(3), unflat(0), unflat(4), unflat(13), unflat(20), unflat(13)]
    assert got['score'][:, 0].tolist() == [[-0.5, 0.25], [-0.5, 0.0], [-0.5, 0.0], [0.0, 0.0], [-inf, 0.125], [0.0, 0.0]]
    for i in (3, 5):
        assert got['theta'][i].view(np.int32) == theta[i].view(np.int32) and np.array_equal(_bits(got['dx'][i]), _bits(dx[i]))
    same(got, SR.select_ref(table, ppc, yy, np.zeros((6, 1), dtype=np.int64), theta, dx, n, K, A, S, 1.0, 0.05))


@pytest.mark.parametrize('per_shift', [0, 1])
def test_invalid_slots(per_shift):
    """Slots of -1 and K are skipped with scores (0, 0), and nothing of their rows is read: the rows hold 1e30, which would win.
    An image with no valid slot keeps its pose bit for bit and its slot-0 value."""
    A, S, K, n, M = 1, 1, 3, 16, 3
    c = random_tables(4, M, A, S, K, 9)
    c['cand'] = np.array([[-1, 1, K], [K, -1, 2], [-1, K, -1], [K, K, K]])
    dead = ~((c['cand'] >= 0) & (c['cand'] < K))
    c['num'][dead] = 1e30
    pp = c['pp'] if per_shift else c['ppc']
    got = run_select(c['theta'], c['dx'], c['cand'], c['num'], pp, c['yy'], n, K, A, S)
    assert got['cls'].tolist() == [1, 2, -1, K] and got['best'][:, 0].tolist() == [1, 2, 0, 0]
    assert not got['score'][dead].any() and (np.abs(got['score'][~dead]) < 1e3).all()
    assert not got['best'][2:].any()
    assert np.array_equal(_bits(got['theta'][2:]), _bits(c['theta'][2:])) and np.array_equal(_bits(got['dx'][2:]), _bits(c['dx'][2:]))
    same(got, SR.select_ref(c['num'], pp, c['yy'], c['cand'], c['theta'], c['dx'], n, K, A, S, 1.0, 0.05))


def test_rows_do_not_depend_on_the_call():
    N, M, A, S, K, n = 11, 3, 2, 1, 4, 16
    c = random_tables(N, M, A, S, K, 21)
    whole = run_select(c['theta'], c['dx'], c['cand'], c['num'], c['ppc'], c['yy'], n, K, A, S)
    for lo, hi in ((0, 3), (3, 4), (4, 11)):
        part = run_select(c['theta'][lo:hi], c['dx'][lo:hi], c['cand'][lo:hi], c['num'][lo:hi], c['ppc'][lo:hi], c['yy'][lo:hi], n, K, A, S)
        same(part, {k: v[lo:hi] for k, v in whole.items()})


# ---- 3. agreement with the kernels that select from their own tables -------------------------------------------------------------------
def test_per_shift_power_is_pose_classify_and_pose_refine():
    from tvae import _cluster_lib as CL
    N, C, n, K, M, A, S = 6, 2, 9, 3, 3, 1, 1
    rng = np.random.default_rng(17)
    Y, refs = rng.standard_normal((N, C, n, n)).astype(F32), rng.standard_normal((K, C, n, n)).astype(F32)
    theta, dx = rng.uniform(-3, 3, N).astype(F32), rng.uniform(-0.1, 0.1, (N, 2)).astype(F32)
    cand = np.array([[0, 1, 2], [2, 2, 0], [1, -1, 0], [K, 0, 1], [-1, K, -1], [2, 1, 0]])
    t, dth, radius, edge = 1.25, 0.07, 3.0, 1.5
    cnd = (2 * A + 1) * (2 * S + 1) ** 2
    wsf = CL.query('tvae_pose_classify_ws_floats', N, M, C, n, A, S)
    o = dict(cls=torch.empty(N, dtype=torch.int32, device=DEV), best=torch.empty(N, 4, dtype=torch.int32, device=DEV),
             theta=torch.empty(N, device=DEV), dx=torch.empty(N, 2, device=DEV), score=torch.empty(N, M, 2, device=DEV))
    num, pp, yy = torch.empty(N, M, 3, 3, 3, device=DEV), torch.empty(N, M, 3, 3, 3, device=DEV), torch.empty(N, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_classify', _dev(Y), _dev(theta), _dev(dx), _dev(cand, torch.int32), _dev(refs), *o.values(), num, pp, yy,
                torch.empty(wsf, device=DEV), wsf, N, C, n, K, M, A, S, t, dth, radius, edge)
    got = run_select(theta, dx, cand, num.cpu().numpy(), pp.cpu().numpy(), yy.cpu().numpy(), n, K, A, S, t, dth)
    same(got, {k: v.cpu().numpy() for k, v in o.items()})
    # tvae_pose_refine: the tables of one slot
    cls = np.array([0, 2, 1, -1, K, 1])
    wsf = CL.query('tvae_pose_refine_ws_floats', N, C, n, A, S)
    r = dict(theta=torch.empty(N, device=DEV), dx=torch.empty(N, 2, device=DEV), score=torch.empty(N, 2, device=DEV),
             best=torch.empty(N, 3, dtype=torch.int32, device=DEV))
    num, pp = torch.empty(N, cnd, device=DEV), torch.empty(N, cnd, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_refine', _dev(Y), _dev(theta), _dev(dx), _dev(cls, torch.int32), _dev(refs), *r.values(), num, pp, yy,
                torch.empty(wsf, device=DEV), wsf, N, C, n, K, A, S, t, dth, radius, edge)
    shape = (N, 1, 3, 3, 3)
    got = run_select(theta, dx, cls[:, None], num.cpu().numpy().reshape(shape), pp.cpu().numpy().reshape(shape), yy.cpu().numpy(), n, K, A,
                     S, t, dth)
    want = {k: v.cpu().numpy() for k, v in r.items()}
    same(dict(theta=got['theta'], dx=got['dx'], score=got['score'][:, 0], best=got['best'][:, 1:]), want, ('theta', 'dx', 'score', 'best'))
    assert got['cls'].tolist() == cls.tolist() and not got['best'][:, 0].any()


# ---- 4. rejections ---------------------------------------------------------------------------------------------------------------------
def test_rejections():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    N, M, A, S, K, n = 5, 3, 2, 1, 4, 16
    c = random_tables(N, M, A, S, K, 2)
    base = dict(theta=c['theta'], dx=c['dx'], cand=c['cand'], num=c['num'], pp=c['ppc'], yy=c['yy'], n=n, K=K, A=A, S=S)
    bad = [dict(per_shift=2), dict(per_shift=-1), dict(M=65), dict(M=0), dict(S=9), dict(S=-1), dict(A=33), dict(A=-1), dict(n=1),
           dict(n=129), dict(N=0), dict(N=(1 << 24) + 1), dict(K=0), dict(K=65536), dict(t=float('nan')), dict(t=float('inf')),
           dict(t=0.0), dict(t=-1.0), dict(dtheta=float('nan')), dict(dtheta=float('inf'))]
    for kw in bad:
        with pytest.raises(TvaeHipError, match='tvae_pose_select failed with hipError_t 1'):
            run_select(**dict(base, **kw))
        assert untouched(run_select.last), kw
    # N M NA NS^2 = 2^24 * 64 * 65 * 289 is beyond 2^40 (the pointers are never followed: the call is rejected on the host)
    with pytest.raises(TvaeHipError, match='hipError_t 1'):
        run_select(**dict(base, A=32, S=8), N=1 << 24, M=64)
    assert untouched(run_select.last)
    # an output that overlaps an input, and two outputs that overlap
    t = {k: _dev(v) for k, v in c.items() if k not in ('cand', 'pp')}
    cand = _dev(c['cand'], torch.int32)
    o = dict(cls=torch.full((N,), SENT_I, dtype=torch.int32, device=DEV), best=torch.full((N, 4), SENT_I, dtype=torch.int32, device=DEV),
             theta=torch.full((N,), SENT_F, device=DEV), dx=torch.full((N, 2), SENT_F, device=DEV),
             score=torch.full((N, M, 2), SENT_F, device=DEV))
    tail = (N, n, K, M, A, S, 0, 1.0, 0.05)
    flat = torch.full((3 * N - 2,), SENT_F, device=DEV)       # theta_out begins inside dx
    both = torch.full((5 * N - 1,), SENT_I, dtype=torch.int32, device=DEV)        # best begins at the last word of cls_out
    calls = [(t['theta'], flat[:2 * N].view(N, 2), cand, t['num'], t['ppc'], t['yy'], o['cls'], o['best'], flat[2 * N - 2:], o['dx'], o['score']),
             (t['theta'], t['dx'], cand, t['num'], t['ppc'], t['yy'], both[:N], both[N - 1:].view(N, 4), o['theta'], o['dx'], o['score']),
             (t['theta'], t['dx'], cand, t['num'], t['ppc'], t['num'].view(-1)[:N], o['cls'], o['best'], o['theta'], o['dx'],
              t['num'].view(-1)[8:8 + 2 * N * M].view(N, M, 2))]                   # score inside num
    for args in calls:
        with pytest.raises(TvaeHipError, match='hipError_t 1'):
            with guardband.GuardedCalls():
                CL.call('tvae_pose_select', *args, *tail)
    assert bool((flat == SENT_F).all()) and bool((both == SENT_I).all()) and torch.equal(t['num'], _dev(c['num']))
    assert untouched({k: v.cpu().numpy() for k, v in o.items()})


# ---- 5. the wrappers against the hand composition of their parts -------------------------------------------------------------------------
def _stack(N=10, n=12, K=2, A=1, S=1, seed=5):
    p = R.planted_ctf(0.3, 4, seed, N=N, n=n, K=K, A=A, S=S)
    p['cls'][N - 1] = -1                                       # one image outside every class
    return p


def _count_selects(monkeypatch):
    from tvae import ctf
    calls, inner = [], ctf.select_poses
    monkeypatch.setattr(ctf, 'select_poses', lambda *a, **k: (calls.append(a[2].numel()), inner(*a, **k))[1])
    return calls


@pytest.mark.parametrize('pieces', [1, 3])
def test_classify_poses_with_ctf_is_the_composition(pieces, monkeypatch):
    from tvae import classify, ctf, ml2d, refine
    p = _stack()
    N, n, K, A, S, t, step = p['N'], p['n'], p['K'], p['A'], p['S'], p['t'], 0.06
    M, cnd = 2, (2 * A + 1) * (2 * S + 1) ** 2
    Y, th, d, refs = _dev(p['Y']), _dev(p['theta']), _dev(p['dx']), _dev(p['refs'])
    cand = np.stack([p['cls'], np.where(p['cls'] >= 0, 1 - p['cls'], K)], 1)
    coef = _dev(p['coef'], torch.float64)
    with guardband.GuardedCalls(replay=True):
        Yf = ctf.filter_stack(Y, coef=coef, mode='multiply')
        yy = ml2d.raw_sum_squares(Y)
        num = classify.classify_poses(Yf, th, d, cand, refs, t, A, step, S, 4.5, 1.0, tables=True)[5]
        ppc = ctf.template_power(th, d, cand, refs, coef, t, A, step, 4.5, 1.0)
    want = SR.select_ref(num.cpu().numpy(), ppc.cpu().numpy(), yy.cpu().numpy(), cand, p['theta'], p['dx'], n, K, A, S, t, step)
    if pieces == 3:                                            # 4 + 4 + 2 images
        monkeypatch.setattr(refine, 'WS_FLOATS', 4 * (2 * M * cnd + 1))
    calls = _count_selects(monkeypatch)
    with guardband.GuardedCalls(replay=True):
        out = classify.classify_poses(Yf, th, d, cand, refs, t, A, step, S, 4.5, 1.0, tables=True, ctf=(coef, yy))
    assert calls == ([N] if pieces == 1 else [4, 4, 2])
    assert out[0].dtype == torch.int64
    got = dict(cls=out[0].cpu().numpy().astype(np.int32), theta=out[1].cpu().numpy(), dx=out[2].cpu().numpy(),
               score=out[3].cpu().numpy(), best=out[4].cpu().numpy())
    same(got, want)
    assert torch.equal(out[5], num) and torch.equal(out[6], ppc) and torch.equal(out[7], yy)
    # without tables: the five results alone; and the thin wrapper, with the power in either shape
    with guardband.GuardedCalls(replay=True):
        assert len(classify.classify_poses(Yf, th, d, cand, refs, t, A, step, S, 4.5, 1.0, ctf=(coef, yy))) == 5
        a = ctf.select_poses(num, ppc, yy, cand, th, d, n, K, t, A, step, S)
        b = ctf.select_poses(num, ppc[..., None, None].expand(-1, -1, -1, 3, 3).contiguous(), yy, cand, th, d, n, K, t, A, step, S)
    for x, y, z in zip(a, b, out[:5]):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize('pieces', [1, 3])
def test_refine_poses_with_ctf_is_the_composition(pieces, monkeypatch):
    from tvae import ctf, ml2d, refine
    p = _stack()
    N, n, K, A, S, t, step = p['N'], p['n'], p['K'], p['A'], p['S'], p['t'], 0.06
    cnd = (2 * A + 1) * (2 * S + 1) ** 2
    Y, th, d, refs = _dev(p['Y']), _dev(p['theta']), _dev(p['dx']), _dev(p['refs'])
    coef = _dev(p['coef'], torch.float64)
    with guardband.GuardedCalls(replay=True):
        Yf = ctf.filter_stack(Y, coef=coef, mode='multiply')
        yy = ml2d.raw_sum_squares(Y)
        num = refine.refine_poses(Yf, th, d, p['cls'], refs, t, A, step, S, tables=True)[4]
        ppc = ctf.template_power(th, d, p['cls'][:, None], refs, coef, t, A, step)
    want = SR.select_ref(num.cpu().numpy()[:, None], ppc.cpu().numpy(), yy.cpu().numpy(), p['cls'][:, None], p['theta'], p['dx'], n, K, A,
                         S, t, step)
    if pieces == 3:
        monkeypatch.setattr(refine, 'WS_FLOATS', 4 * (2 * cnd + 1))
    calls = _count_selects(monkeypatch)
    with guardband.GuardedCalls(replay=True):
        out = refine.refine_poses(Yf, th, d, p['cls'], refs, t, A, step, S, tables=True, ctf=(coef, yy))
    assert calls == ([N] if pieces == 1 else [4, 4, 2])
    assert tuple(out[2].shape) == (N, 2) and tuple(out[3].shape) == (N, 3) and tuple(out[5].shape) == (N, 2 * A + 1)
    got = dict(theta=out[0].cpu().numpy(), dx=out[1].cpu().numpy(), score=out[2].cpu().numpy(), best=out[3].cpu().numpy())
    same(got, dict(theta=want['theta'], dx=want['dx'], score=want['score'][:, 0], best=want['best'][:, 1:]), ('theta', 'dx', 'score', 'best'))
    assert torch.equal(out[4], num) and torch.equal(out[5], ppc[:, 0]) and torch.equal(out[6], yy)
    with guardband.GuardedCalls(replay=True):
        assert len(refine.refine_poses(Yf, th, d, p['cls'], refs, t, A, step, S, ctf=(coef, yy))) == 4


# ---- 6. the rounds -----------------------------------------------------------------------------------------------------------------------
def _rounds_case():
    p = R.planted_ctf(0.3, 4, 8, N=24, n=12, K=2, A=1, S=1)
    return p, _dev(p['Y']), _dev(p['theta']), _dev(p['dx'])


@pytest.mark.parametrize('cross', [False, True])
def test_rounds_without_ctf_are_the_rounds_without_the_argument(cross):
    from tvae import classify, refine
    p, Y, th, d = _rounds_case()
    args = (p['K'], p['t'], 2, 0.1, p['A'], p['S'], None, 0.0, cross)
    with guardband.GuardedCalls(replay=True):
        a = refine.refine_rounds(Y, th, d, p['cls'], *args)
        b = refine.refine_rounds(Y, th, d, p['cls'], *args, ctf=None, wiener_tau=0.3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2]['scores'], b[2]['scores'])
    assert sorted(a[2]) == sorted(b[2]) == ['scores', 'steps']
    with guardband.GuardedCalls(replay=True):
        a = classify.classify_rounds(Y, th, d, p['cls'], *args)
        b = classify.classify_rounds(Y, th, d, p['cls'], *args, ctf=None, wiener_tau=0.3)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and torch.equal(a[3]['slot_scores'], b[3]['slot_scores'])
    assert sorted(a[3]) == sorted(b[3]) and 'ctf_power' not in b[3]


def _half_labels(cls, K):
    """h K + k for an image at position parity h among the members of class k in ascending image index; -1 outside [0, K)."""
    out = np.full(cls.size, -1, dtype=np.int64)
    for k in range(K):
        members = np.flatnonzero(cls == k)
        out[members] = k + K * (np.arange(members.size) % 2)
    return out


@pytest.mark.parametrize('tool', ['refine', 'classify'])
def test_rounds_with_ctf_and_cross_halves_score_against_the_other_half(tool):
    """One round, so that the references are those of the input labels and poses: recomputed here from half-set labels built in
    numpy, they are the history's bit for bit; every slot of an image's own class names the half the image is NOT in, and that
    reference does not change by a bit when the image is taken out of the stack's labels."""
    from tvae import classify, ctf, refine
    p, Y, th, d = _rounds_case()
    N, K, n, t, tau = p['N'], p['K'], p['n'], p['t'], 0.2
    cls = p['cls'].copy()
    cls[5] = -1
    args = (K, t, 1, 0.1, p['A'], p['S'], None, 0.0, True)
    with guardband.GuardedCalls(replay=True):
        if tool == 'refine':
            th1, d1, hist = refine.refine_rounds(Y, th, d, cls, *args, ctf=p['coef'], wiener_tau=tau)
            lab1 = torch.from_numpy(cls).to(DEV)
            members = hist['members']
        else:
            lab1, th1, d1, hist = classify.classify_rounds(Y, th, d, cls, *args, ctf=p['coef'], wiener_tau=tau)
            members = hist['members']
    inside = _half_labels(cls, K)
    with guardband.GuardedCalls(replay=True):
        refs = ctf.class_averages_ctf(Y, th, d, inside, p['coef'], 2 * K, t, 'wiener', tau)[0]
    assert torch.equal(hist['references'], refs)
    slots = hist['slots'].cpu().numpy().reshape(N, -1)
    own = slots[:, 0]
    assert np.array_equal(own, np.where(inside >= 0, (inside + K) % (2 * K), -1))       # the own class: the other half
    assert not (slots == inside[:, None])[inside >= 0].any()                       # no slot names the half the image is in
    for i in (0, 1, 7, 12):
        without = inside.copy()
        without[i] = -1
        with guardband.GuardedCalls(replay=True):
            r = ctf.class_averages_ctf(Y, th, d, without, p['coef'], 2 * K, t, 'wiener', tau)[0]
        for s in slots[i][slots[i] >= 0]:
            assert torch.equal(r[s], refs[s]), (i, s)
        assert not torch.equal(r[inside[i]], refs[inside[i]])
    # what comes back: the Wiener averages of the final labels and poses, and their power
    with guardband.GuardedCalls(replay=True):
        avg, m, D = ctf.class_averages_ctf(Y, th1, d1, lab1, p['coef'], K, t, 'wiener', tau)
    assert torch.equal(hist['averages'], avg) and torch.equal(members, m) and torch.equal(hist['ctf_power'], D)
    assert tuple(D.shape) == (K, n, n // 2 + 1) and bool(torch.isfinite(avg).all())
    assert np.isfinite(hist['scores']).all()


# ---- 7. the scripts ------------------------------------------------------------------------------------------------------------------------
def test_refine_poses_py_and_reclassify_particles_py_with_ctf(tmp_path):
    """Both scripts with --ctf from the files a clustering run writes: the files of a plain run plus the per-class power, and the
    poses, labels and averages of the library call with the same arguments."""
    from tvae import classify, ctf, refine
    N, n, K = 12, 16, 2
    p = R.planted_ctf(0.2, 4, 13, N=N, n=n, K=K, A=2, S=1)
    rng = np.random.default_rng(14)
    tab = np.zeros((N, 8))
    tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3], tab[:, 4], tab[:, 5] = rng.uniform(1.0, 3.0, N), 2.7, 300.0, 1.2, 100.0, 7.0
    files = {}
    for name, arr in (('stack', p['Y'][:, 0]), ('rotations', p['theta'].reshape(N, 1)), ('translations', p['dx']), ('clusters', p['cls']),
                      ('latents', rng.standard_normal((N, 2)).astype(F32))):
        files[name] = str(tmp_path / (name + '.npy'))
        np.save(files[name], arr)
    np.savetxt(str(tmp_path / 'ctf.txt'), tab)
    common = ['--stack', files['stack'], '--rotations', files['rotations'], '--translations', files['translations'], '--clusters',
              files['clusters'], '--n-clusters', str(K), '--rounds', '2', '--angle-steps', '2', '--shift', '1', '--ctf',
              str(tmp_path / 'ctf.txt'), '--scale', '2', '--wiener-tau', '0.2']

    def run(script, out, extra=()):
        r = subprocess.run([sys.executable, os.path.join(PKG, script), *common, *extra, '--out-dir', str(tmp_path / out)],
                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        return tmp_path / out

    coef = ctf.coefficients(tab, scale=2)
    Y, th, d = _dev(p['Y']), _dev(p['theta']), _dev(p['dx'])
    out = run('refine_poses.py', 'refined')
    want = {'class_averages_refined.npy', 'class_ctf_power_refined.npy', 'refine_scores.npy', 'rotations_refined.npy',
            'translations_refined.npy'}
    assert want <= set(os.listdir(out)) <= want | {'class_averages_refined.jpg'}
    with guardband.GuardedCalls(replay=True):
        th1, d1, hist = refine.refine_rounds(Y, th, d, p['cls'], K, p['t'], 2, np.radians(22.5), 2, 1, ctf=coef, wiener_tau=0.2)
    assert np.array_equal(np.load(out / 'rotations_refined.npy'), th1.cpu().numpy().reshape(N, 1))
    assert np.array_equal(np.load(out / 'translations_refined.npy'), d1.cpu().numpy())
    assert np.array_equal(np.load(out / 'class_averages_refined.npy'), hist['averages'].cpu().numpy())
    assert np.array_equal(np.load(out / 'class_ctf_power_refined.npy'), hist['ctf_power'].cpu().numpy())
    out = run('reclassify_particles.py', 'reclassified', ['--latents', files['latents'], '--candidates', '2'])
    want = {'class_averages_reclassified.npy', 'class_ctf_power_reclassified.npy', 'class_scores.npy', 'classify_moved.npy',
            'classify_scores.npy', 'clusters_reclassified.npy', 'rotations_reclassified.npy', 'translations_reclassified.npy'}
    assert want <= set(os.listdir(out)) <= want | {'class_averages_reclassified.jpg'}
    with guardband.GuardedCalls(replay=True):
        lab2, th2, d2, hist = classify.classify_rounds(Y, th, d, p['cls'], K, p['t'], 2, np.radians(22.5), 2, 1,
                                                       latents=np.load(files['latents']), candidates=2, ctf=coef, wiener_tau=0.2)
    assert np.array_equal(np.load(out / 'clusters_reclassified.npy'), lab2.cpu().numpy())
    assert np.array_equal(np.load(out / 'translations_reclassified.npy'), d2.cpu().numpy())
    assert np.array_equal(np.load(out / 'class_averages_reclassified.npy'), hist['averages'].cpu().numpy())
    assert np.array_equal(np.load(out / 'class_ctf_power_reclassified.npy'), hist['ctf_power'].cpu().numpy())
