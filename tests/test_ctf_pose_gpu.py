"""The CTF in the template on the GPU: tvae_template_ctf_power and tvae_ctf_power_entries behind their C ABI (every call under
guard bands with replay, outputs and workspace filled with a sentinel) against the fp64 restatement tests/ctf_pose_ref.py, then
tvae.ctf.template_power / power_weighted and tvae.ml2d.ml_rounds(ctf=...).

Tolerances.  template power: the a-priori bound of tests/ctf_pose_ref.py (its docstring derives it; test_ctf_pose_ref_cpu.py
checks without the kernel that the float32 restatement stays inside it and that it is at most 1 % of the reference on every
case).  H = 1: both kernels against the same fp64 sum of T^2, the bound of tvae_pose_classify's pp (test_refine_gpu.py) plus
that of the template power.  tvae_ctf_power_entries: 1e-15 relative for the fp64 sums plus the contract of tvae_ctf_eval,
sum w (2 |H| dH + dH^2) with dH = 8 2^-24 (|c0| + |c1|).  The loop: tests/ctf_pose_ref.py, `loop_tolerance`."""
import functools

import numpy as np
import pytest
import torch

import align_ref
import ctf_pose_ref as R
import ctf_ref
import guardband

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 2.0 ** -24
SENT_F = -12345.5
SENT_I = -7777777


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


# ---- the C ABI under guard bands -----------------------------------------------------------------------------------------------------
def run_power(theta, dx, cand, refs, coef, A, t, dtheta, radius=0.0, edge=0.0, K=None, N=None, C=None, n=None, M=None,
              ws_short=0, ref_dev=None):
    """tvae_template_ctf_power into a sentinel-filled output and workspace -> fp32 numpy [N][M][NA]."""
    from tvae import _cluster_lib as CL
    cand = np.asarray(cand)
    N = cand.shape[0] if N is None else N
    M = cand.shape[1] if M is None else M
    K = refs.shape[0] if K is None else K
    C = refs.shape[1] if C is None else C
    n = refs.shape[-1] if n is None else n
    rows, slots, NA = max(cand.shape[0], 1), max(cand.shape[1], 1), 2 * max(A, 0) + 1
    out = torch.full((rows, slots, NA), SENT_F, device=DEV)
    ws = torch.full((1,), SENT_F, dtype=torch.float64, device=DEV).view(torch.float32)
    try:
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_template_ctf_power', _dev(theta), _dev(dx), _dev(cand, torch.int32),
                    _dev(refs) if ref_dev is None else ref_dev, _dev(coef, torch.float64), out, ws, 2 - ws_short, N, C, n, K, M, A,
                    float(t), float(dtheta), float(radius), float(edge))
    finally:
        run_power.last = (out.cpu().numpy(), ws.cpu().numpy())
    assert np.array_equal(run_power.last[1].view(np.float64), [SENT_F])   # the workspace is never touched
    return out.cpu().numpy()


def run_weighted(coef, img, w, seg, n, N=None, E=None, K=None):
    from tvae import _cluster_lib as CL
    N = np.asarray(coef).shape[0] if N is None else N
    E = len(img) if E is None else E
    K = len(seg) - 1 if K is None else K
    R_ = n // 2 + 1
    D = torch.full((max(len(seg) - 1, 1), n, R_), SENT_F, dtype=torch.float64, device=DEV)
    wsum = torch.full((max(len(seg) - 1, 1),), SENT_F, dtype=torch.float64, device=DEV)
    counts = torch.full((max(len(seg) - 1, 1),), SENT_I, dtype=torch.int32, device=DEV)
    try:
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_ctf_power_entries', _dev(coef, torch.float64), _dev(img, torch.int32), _dev(w), _dev(seg, torch.int32),
                    D, wsum, counts, N, E, K, n)
    finally:
        run_weighted.last = (D.cpu().numpy(), wsum.cpu().numpy(), counts.cpu().numpy())
    return run_weighted.last


@functools.lru_cache(maxsize=None)
def case(geometry):
    c = dict(R.gpu_case(*geometry))
    c['got'] = run_power(c['theta'], c['dx'], c['cand'], c['refs'], c['coef'], c['A'], c['t'], c['dtheta'], c['radius'], c['edge'])
    c['got'].setflags(write=False)
    return c


# ---- 1. template power ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', R.GPU_CASES)
def test_template_power_against_fp64(geometry):
    """Against ctf_pose_ref.template_power within its a-priori bound.  Measured on an MI355X: the largest |got - ref| is between
    6.9e-5 and 5.1e-4 of the bound over the ten cases, 1.4e-7 to 4.6e-7 of the reference."""
    c = case(geometry)
    got, ref, bound = c['got'].astype(np.float64), c['ref'], c['bound']
    valid = (c['cand'] >= 0) & (c['cand'] < R.K_CLS)
    err = np.abs(got - ref)
    print(f'{geometry}: largest |got - ref| / bound {(err[valid] / bound[valid]).max():.3e}, / ref {(err[valid] / ref[valid]).max():.3e}')
    assert not got[~valid].any()                              # an invalid slot: exact zeros
    assert (err <= bound).all()
    if c['M'] == 3:                                           # the duplicate slots of row 1 are the same bits
        assert np.array_equal(c['got'][1, 0], c['got'][1, 1])


@pytest.mark.parametrize('geometry', [(9, 2, 3, 2, True), (33, 1, 3, 2, True), (64, 2, 1, 2, False), (128, 1, 1, 0, True)])
def test_unit_transfer_is_the_centre_pp_of_pose_classify(geometry):
    """coef = (0, 1, 0, 0, 0): H = 1 exactly (cos 0 and exp 0 are exact), so ppc is the sum of T^2 -- what tvae_pose_classify
    writes as pp at the centre shift for the same inputs.  Both within their own bounds of the fp64 sum."""
    from tvae import _cluster_lib as CL
    c = case(geometry)
    n, C, M, A = c['n'], c['C'], c['M'], c['A']
    N, S, NA = R.N_IMG, 1, 2 * A + 1
    coef = np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (N, 1))
    got = run_power(c['theta'], c['dx'], c['cand'], c['refs'], coef, A, c['t'], c['dtheta'], c['radius'], c['edge'])
    want = (c['T'] ** 2).sum((-3, -2, -1))
    b = R.sample_bound(c['refs'], c['cand'], c['dx'], c['t'], c['radius'] if c['radius'] > 0 else None, c['edge'])
    b1 = R.template_power_bound(c['T'], coef, b)
    assert (np.abs(got - want) <= b1).all()
    rng = np.random.default_rng(n)
    Y = rng.standard_normal((N, C, n, n)).astype(np.float32)
    wsf = CL.query('tvae_pose_classify_ws_floats', N, M, C, n, A, S)
    ws = torch.empty(wsf, device=DEV)
    num, pp = (torch.full((N, M, NA, 3, 3), SENT_F, device=DEV) for _ in range(2))
    yy = torch.full((N,), SENT_F, device=DEV)
    outs = (torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, 4, dtype=torch.int32, device=DEV),
            torch.empty(N, device=DEV), torch.empty(N, 2, device=DEV), torch.empty(N, M, 2, device=DEV))
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_pose_classify', _dev(Y), _dev(c['theta']), _dev(c['dx']), _dev(c['cand'], torch.int32), _dev(c['refs']), *outs,
                num, pp, yy, ws, wsf, N, C, n, R.K_CLS, M, A, S, float(c['t']), float(c['dtheta']), float(c['radius']),
                float(c['edge']))
    centre = pp[:, :, :, S, S].cpu().numpy().astype(np.float64)
    b2 = R.pp_bound(c['T'], R.sample_bound(c['refs'], c['cand'], c['dx'], c['t'], c['radius'] if c['radius'] > 0 else None,
                                           c['edge'], S=S))
    assert (np.abs(centre - want) <= b2).all()
    assert (np.abs(got - centre) <= b1 + b2).all()


def test_edge_rows():
    """A NaN or out-of-frame pose gives a row of exact zeros; a slot outside [0, K) gives zeros and reads nothing: the planes
    around the valid references are NaN, so a read of plane -1 or K would show."""
    n, C, M, A, K = 16, 2, 3, 1, 2
    rng = np.random.default_rng(3)
    refs = rng.standard_normal((K, C, n, n)).astype(np.float32)
    theta = np.array([0.1, np.nan, 0.3, 0.4, 0.5], dtype=np.float32)
    dx = np.array([[0.0, 0.0], [0.0, 0.0], [1e30, 0.0], [0.0, np.inf], [np.nan, 0.1]], dtype=np.float32)
    cand = np.array([[0, K, -1], [0, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 0]])
    coef = R.defocus_rows(n, 5, 0.6)
    big = torch.full((K + 2, C, n, n), float('nan'), device=DEV)
    big[1:K + 1] = _dev(refs)
    got = run_power(theta, dx, cand, refs, coef, A, 1.0, 0.05, ref_dev=big[1:K + 1])
    assert (got[0, 0] > 0).all() and np.isfinite(got[0, 0]).all()
    assert not got[0, 1:].any() and not got[1:].any()
    # a non-finite coefficient row stays in its image's row
    coef2 = coef.copy()
    coef2[0, 2] = np.nan
    theta2, dx2 = np.full(5, 0.2, dtype=np.float32), np.zeros((5, 2), dtype=np.float32)
    a = run_power(theta2, dx2, np.zeros((5, 1), dtype=np.int64), refs, coef, A, 1.0, 0.05)
    b = run_power(theta2, dx2, np.zeros((5, 1), dtype=np.int64), refs, coef2, A, 1.0, 0.05)
    assert np.isnan(b[0]).all() and np.array_equal(a[1:], b[1:])


@pytest.mark.parametrize('geometry', [(9, 2, 3, 2, True), (64, 1, 3, 0, True)])
def test_bits(geometry):
    """Two runs are equal; a row does not depend on N, on the other rows or on where it stands in the call."""
    c = case(geometry)
    args = (c['A'], c['t'], c['dtheta'], c['radius'], c['edge'])
    again = run_power(c['theta'], c['dx'], c['cand'], c['refs'], c['coef'], *args)
    assert np.array_equal(again, c['got'])
    rev = np.arange(R.N_IMG)[::-1].copy()
    back = run_power(c['theta'][rev], c['dx'][rev], c['cand'][rev], c['refs'], c['coef'][rev], *args)
    assert np.array_equal(back[rev], c['got'])
    for i in (0, 3):
        one = run_power(c['theta'][i:i + 1], c['dx'][i:i + 1], c['cand'][i:i + 1], c['refs'], c['coef'][i:i + 1], *args)
        assert np.array_equal(one[0], c['got'][i])
    # more references behind the ones the rows name change nothing
    more = np.concatenate([c['refs'], c['refs'][:1] + 1])
    cand = np.where((c['cand'] >= 0) & (c['cand'] < R.K_CLS), c['cand'], -1)
    assert np.array_equal(run_power(c['theta'], c['dx'], cand, more, c['coef'], *args), c['got'])


def test_rejections():
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    c = R.gpu_case(16, 1, 3, 2, False)
    base = dict(theta=c['theta'], dx=c['dx'], cand=c['cand'], refs=c['refs'], coef=c['coef'], A=2, t=1.0, dtheta=0.05)
    bad = [dict(N=0), dict(N=(1 << 24) + 1), dict(C=0), dict(C=17), dict(n=1), dict(n=129), dict(K=0), dict(K=65536), dict(M=0),
           dict(M=65), dict(A=-1), dict(A=33), dict(t=0.0), dict(t=float('nan')), dict(t=float('inf')), dict(dtheta=float('nan')),
           dict(radius=float('nan')), dict(edge=-1.0), dict(edge=float('inf')), dict(ws_short=1)]
    for kw in bad:
        with pytest.raises(TvaeHipError, match='hipError_t 1'):
            run_power(**dict(base, **kw))
        assert (run_power.last[0] == SENT_F).all(), kw
    for args in [(0, 1, 16, 3, 2), (5, 0, 16, 3, 2), (5, 17, 16, 3, 2), (5, 1, 1, 3, 2), (5, 1, 129, 3, 2), (5, 1, 16, 0, 2),
                 (5, 1, 16, 65, 2), (5, 1, 16, 3, -1), (5, 1, 16, 3, 33), (1 << 24, 1, 16, 64, 1)]:
        assert CL.query('tvae_template_ctf_power_ws_floats', *args) == 0, args
    assert CL.query('tvae_template_ctf_power_ws_floats', 5, 1, 16, 3, 2) == 2
    # an output that overlaps an input
    th = _dev(np.zeros(80, dtype=np.float32))
    with pytest.raises(TvaeHipError, match='hipError_t 1'):
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_template_ctf_power', th[:5], _dev(c['dx']), _dev(c['cand'], torch.int32), _dev(c['refs']),
                    _dev(c['coef'], torch.float64), th[:75].view(5, 3, 5), torch.zeros(2, device=DEV), 2, 5, 1, 16, R.K_CLS, 3, 2,
                    1.0, 0.05, 0.0, 0.0)
    assert not th.any()
    # tvae_ctf_power_entries
    coef, img, w, seg = c['coef'], np.arange(5), np.ones(5, dtype=np.float32), np.array([0, 2, 5])
    for kw in [dict(n=1), dict(n=1025), dict(N=0), dict(N=(1 << 24) + 1), dict(E=0), dict(E=(1 << 30) + 1), dict(K=0), dict(K=65536)]:
        with pytest.raises(TvaeHipError, match='hipError_t 1'):
            run_weighted(coef, img, w, seg, **dict(dict(n=8), **kw))
        D, wsum, counts = run_weighted.last
        assert (D == SENT_F).all() and (wsum == SENT_F).all() and (counts == SENT_I).all(), kw


# ---- 2. the weighted power ---------------------------------------------------------------------------------------------------------------
def _entries(n, N, K, E, seed):
    rng = np.random.default_rng(seed)
    coef = R.defocus_rows(n, N, 0.3)
    cls = np.sort(rng.integers(0, K, E))
    seg = np.searchsorted(cls, np.arange(K + 1))
    return coef, rng.integers(0, N, E), rng.uniform(0.01, 1.0, E).astype(np.float32), seg


@pytest.mark.parametrize('n,N,K,E', [(9, 7, 3, 40), (16, 5, 1, 300), (33, 12, 4, 90)])
def test_weighted_power_against_fp64(n, N, K, E):
    coef, img, w, seg = _entries(n, N, K, E, n)
    D, wsum, counts = run_weighted(coef, img, w, seg, n)
    ref = R.power_weighted(coef, img, w, seg, n)
    assert (np.abs(D - ref[0]) <= R.power_weighted_bound(coef, img, w, seg, n)).all()
    assert (np.abs(wsum - ref[1]) <= 1e-15 * ref[1]).all() and counts.tolist() == ref[2].tolist()
    # dead entries change nothing, bit for bit: w = 0, NaN, -1, inf and an image outside [0, N), spliced into class 0
    dead_w = np.array([0.0, np.nan, -1.0, np.inf, 1.0, 1.0], dtype=np.float32)
    dead_i = np.array([0, 1, 2, 3, -1, N])
    at = int(seg[1]) // 2
    img2, w2 = np.insert(img, at, dead_i), np.insert(w, at, dead_w)
    seg2 = np.concatenate([[seg[0]], seg[1:] + dead_w.size])
    D2, wsum2, counts2 = run_weighted(coef, img2, w2, seg2, n)
    assert np.array_equal(D2, D) and np.array_equal(wsum2, wsum) and np.array_equal(counts2, counts)
    # class k alone: independent of K and of the other classes
    k = K - 1
    Dk, wk, ck = run_weighted(coef, img[seg[k]:seg[k + 1]], w[seg[k]:seg[k + 1]], [0, seg[k + 1] - seg[k]], n)
    assert np.array_equal(Dk[0], D[k]) and wk[0] == wsum[k] and ck[0] == counts[k]


def test_weighted_power_with_unit_weights_is_ctf_power():
    from tvae import _cluster_lib as CL
    n, N, K = 24, 40, 3
    rng = np.random.default_rng(8)
    coef = R.defocus_rows(n, N, 0.3)
    lab = rng.integers(0, K, N)
    order, seg, _ = align_ref.segments(lab, K)
    D, wsum, counts = run_weighted(coef, order, np.ones(N, dtype=np.float32), seg, n)
    D0 = torch.empty(K, n, n // 2 + 1, dtype=torch.float64, device=DEV)
    c0 = torch.empty(K, dtype=torch.int32, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_ctf_power', _dev(coef, torch.float64), _dev(order, torch.int32), _dev(seg, torch.int32), D0, c0, N, K, n)
    assert np.array_equal(D, D0.cpu().numpy()) and counts.tolist() == c0.tolist() and wsum.tolist() == counts.astype(float).tolist()


def test_broken_seg_is_clamped_on_the_device():
    n, N, E = 8, 4, 10
    coef, img, w, _ = _entries(n, N, 1, E, 1)
    for seg in ([5, -3, 99, 2], [-7, 4, 4, 1 << 30], [E + 5, 0, 3, 7]):
        D, wsum, counts = run_weighted(coef, img, w, seg, n)          # (the guard bands are the check that nothing strays)
        ref = R.power_weighted(coef, img, w, seg, n)
        assert (np.abs(D - ref[0]) <= R.power_weighted_bound(coef, img, w, seg, n)).all() and counts.tolist() == ref[2].tolist()


# ---- 3. the wrappers and the loop -----------------------------------------------------------------------------------------------------
def test_python_wrappers_are_bitwise_the_c_abi():
    from tvae import ctf
    c = case((16, 1, 3, 2, False))
    with guardband.GuardedCalls(replay=True):
        ppc = ctf.template_power(_dev(c['theta']), _dev(c['dx']), c['cand'], _dev(c['refs']), c['coef'], c['t'], c['A'], c['dtheta'])
    assert np.array_equal(ppc.cpu().numpy(), c['got'])
    coef, img, w, seg = _entries(9, 7, 3, 40, 9)
    want = run_weighted(coef, img, w, seg, 9)
    ent = dict(img=_dev(img, torch.int32), w=_dev(w), seg=_dev(seg, torch.int32))
    with guardband.GuardedCalls(replay=True):
        D, wsum, counts = ctf.power_weighted(coef, ent, 9, 3)
    assert np.array_equal(D.cpu().numpy(), want[0]) and np.array_equal(wsum.cpu().numpy(), want[1])
    assert counts.cpu().numpy().tolist() == want[2].tolist()
    none = dict(img=ent['img'][:0].contiguous(), w=ent['w'][:0].contiguous(), seg=torch.zeros(4, dtype=torch.int32, device=DEV))
    D0, w0, c0 = ctf.power_weighted(coef, none, 9, 3)
    assert not D0.any() and not w0.any() and not c0.any()


def _loop_args(p):
    L = R.LOOP
    return (p['K'], p['t'], L['rounds'], p['A'] * p['dtheta'], p['A'], p['S'], None, 0.0, L['keep'], L['noise'] ** 2)


@functools.lru_cache(maxsize=None)
def loop_run():
    from tvae import ml2d
    p = R.loop_case()
    with guardband.GuardedCalls(replay=True):
        out = ml2d.ml_rounds(_dev(p['Y']), _dev(p['theta']), _dev(p['dx']), p['cls'], *_loop_args(p), ctf=p['coef'],
                             wiener_tau=R.LOOP['tau'])
    return p, out


def test_rounds_without_ctf_are_bitwise_the_rounds_without_the_argument():
    from tvae import ml2d
    p = R.loop_case()
    Y, th, d = _dev(p['Y']), _dev(p['theta']), _dev(p['dx'])
    for cross in (False, True):
        a = ml2d.ml_rounds(Y, th, d, p['cls'], *_loop_args(p), cross_halves=cross)
        b = ml2d.ml_rounds(Y, th, d, p['cls'], *_loop_args(p), cross_halves=cross, ctf=None, wiener_tau=0.3)
        for x, y in zip(a[:5], b[:5]):
            assert torch.equal(x, y)
        assert np.array_equal(a[5]['log_likelihood'], b[5]['log_likelihood']) and 'ctf_power' not in b[5]


def test_rounds_with_ctf_are_reproducible_and_cross_halves_run():
    from tvae import ml2d
    p, (avg, wsum, lab, th, d, hist) = loop_run()
    N, K, n = p['N'], p['K'], p['n']
    assert tuple(avg.shape) == (K, 1, n, n) and bool(torch.isfinite(avg).all())
    assert tuple(hist['ctf_power'].shape) == (K, n, n // 2 + 1) and hist['ctf_power'].dtype == torch.float64
    assert abs(float(wsum.sum()) - N) <= N * 2.0 ** -22
    Y, th0, d0 = _dev(p['Y']), _dev(p['theta']), _dev(p['dx'])
    again = ml2d.ml_rounds(Y, th0, d0, p['cls'], *_loop_args(p), ctf=p['coef'], wiener_tau=R.LOOP['tau'])
    for x, y in zip((avg, wsum, lab, th, d), again[:5]):
        assert torch.equal(x, y)
    # sigma2 = None: the start comes from the same three tables
    est = ml2d.ml_rounds(Y, th0, d0, p['cls'], *_loop_args(p)[:-1], None, ctf=p['coef'], wiener_tau=R.LOOP['tau'])
    assert 0.25 * R.LOOP['noise'] ** 2 < est[5]['sigma2'][0] < 4 * R.LOOP['noise'] ** 2
    with guardband.GuardedCalls(replay=True):
        ch = ml2d.ml_rounds(Y, th0, d0, p['cls'], *_loop_args(p), cross_halves=True, ctf=p['coef'], wiener_tau=R.LOOP['tau'])
    assert bool(torch.isfinite(ch[0]).all()) and abs(float(ch[1].sum()) - N) <= N * 2.0 ** -22
    assert tuple(ch[5]['ctf_power'].shape) == (K, n, n // 2 + 1)


def test_rounds_with_ctf_against_the_reference():
    """Two rounds of ml_rounds(ctf=coef) on the loop case against ctf_pose_ref.rounds in fp64.  The tolerance is that of
    ctf_pose_ref.loop_tolerance, 8 x the error of the float32 restatement of the same loop: the labels and the top-1 poses are
    the reference's for every image whose runner-up margin in the reference clears it (at most 5 % may be left out:
    test_ctf_pose_ref_cpu.py checks the reference alone against that cap), the kept entries are the reference's sets, and the
    averages are within 8 x the float32 restatement's distance from the reference, per class.  Measured on an MI355X:
    |avg - ref|_F 2.40e-6 and 2.50e-6 under tolerances of 1.85e-5 and 2.03e-5, sigma^2 of the second round 0.09376126528 against
    0.09376125783 (the same fp32 value seen through two roundings), one image of 64 left out."""
    p, (avg, wsum, lab, th, d, hist) = loop_run()
    _, ref, tol = R.loop_tolerance()
    keep = ~tol['left_out']
    assert tol['left_out'].mean() <= 0.05 and tol['cut_clear']
    post = hist['posterior']
    assert np.array_equal(np.sort(post['idx'].cpu().numpy(), 1), np.sort(ref['post']['idx'], 1))
    assert np.array_equal(lab.cpu().numpy()[keep], ref['labels'][keep])
    assert np.array_equal(th.cpu().numpy()[keep], ref['theta'][keep]) and np.array_equal(d.cpu().numpy()[keep], ref['dx'][keep])
    err = np.sqrt(((avg.cpu().numpy().astype(np.float64) - ref['avg']) ** 2).sum((1, 2, 3)))
    rel = np.abs(hist['sigma2'] - ref['sigma2']) / ref['sigma2']
    print(f"ml_rounds(ctf): |avg - ref|_F {err.tolist()} of the tolerance {tol['avg'].tolist()}; sigma2 {hist['sigma2'].tolist()} "
          f"against {ref['sigma2'].tolist()}; log-likelihood {hist['log_likelihood'].tolist()} against "
          f"{ref['log_likelihood'].tolist()}")
    assert (err <= tol['avg']).all()
    assert (rel <= 2.0 ** -22).all()                          # both sides round sigma^2 to fp32: a neighbour at the most
    Dref = ref['D']
    assert (np.abs(hist['ctf_power'].cpu().numpy() - Dref) <= 1e-4 * Dref.max()).all()
    assert (np.abs(wsum.cpu().numpy() - ref['wsum']) <= 1e-3 * p['N']).all()
