"""Register-resident attention head (tvae_attn_head_fwd / _bwd with R*P <= 9 * 1024: csrc/small_kernels.hpp,
attn_head_*_reg_kernel) against the strided kernels it replaces -- BITWISE, in one process, the route switched through
TVAE_HEAD_REG -- and against the fp32 oracle restatement of tests/test_hip_primitives.py::test_attn_head (_head_reference: the
oracle's posterior_pool_kl casts to float32) and the float64 one of tests/head_ref.py, both at that test's tolerances.
The calls go through ops.HeadFn (the module API: seven outputs, three of them with optional upstream gradients).

Mid-size reductions with several loads in flight (TVAE_MIDSIZE_ILP: latent_bwd, dec_in_total_img / _sum, part_total_s1,
dft_dbias_rows, enc_tail_wgrad_total) against their one-load-at-a-time forms, bitwise, through their entry points."""
import math
import os
import types

import pytest
import torch

import guardband
from conftest import rel_err

pytestmark = pytest.mark.gpu
B = 3
SPACING = 2.0 / 27
NPT_MAX = 9                        # positions per thread of the largest instance (abi_small.hip: HEAD_REG_MAX_NPT)


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in test_hip_primitives.py: every C-ABI call on relocated tensors between guard bands, twice from the same inputs."""
    with guardband.GuardedCalls(replay=True):
        yield


@pytest.fixture(autouse=True)
def restore_switch():
    old = {k: os.environ.get(k) for k in ('TVAE_HEAD_REG', 'TVAE_MIDSIZE_ILP')}
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _free_tables(R, P, refine):
    """Head tables for any (R, P), P not necessarily a square grid: random but normalised priors (only the bitwise tests use them)."""
    p_r = torch.log_softmax(rnd(R, seed=11), 0)
    return types.SimpleNamespace(
        R=R, P=P, p_r=p_r.to(dev()), off=(rnd(R, seed=12, scale=0.3) if refine else torch.zeros(R)).to(dev()),
        grid=rnd(P, 2, seed=13).contiguous().to(dev()), p_tr=torch.log_softmax(rnd(R * P, seed=14), 0).to(dev()),
        sigma_p=math.pi / R, theta_off_scale=1.0 if refine else 0.0)


def _inputs(RP, zd):
    """Image 0: E at 1e-30 and at 1 - 2^-24 among ordinary draws.  Image 1: every logit shifted by -200 (the softmax is
    shift-invariant: same q as without).  Image 2: every other logit shifted by -200, so that expf(q) == 0 there -- the
    `dead` branch of the KL terms (asserted by the callers)."""
    hd = rnd(3 + 2 * zd, B * RP, seed=1, scale=0.5)
    hd[0] *= 4.0
    hd[0, RP:2 * RP] -= 200.0
    hd[0, 2 * RP + 1:3 * RP:2] -= 200.0
    E = torch.empty(B, RP).exponential_(generator=torch.Generator().manual_seed(2))
    E[0, 0] = 1e-30
    E[0, RP - 1] = 1.0 - 2.0 ** -24
    return hd, E, rnd(B, zd, seed=3), rnd(B, seed=4)


def _run(reg, tb, hd, E, eps_z, eps_t, zd, ups):
    """Forward + backward on one route.  ups: seven upstream gradients, None where absent.  -> (outputs, dheads, PATH_LOG)"""
    from tvae import ops
    os.environ['TVAE_HEAD_REG'] = '1' if reg else '0'
    hg = hd.clone().to(dev()).requires_grad_(True)
    ops.PATH_LOG = set()
    try:
        got = ops.HeadFn.apply(hg, E.to(dev()), eps_z.to(dev()), eps_t.to(dev()), tb, B, zd)
        log = ops.PATH_LOG
    finally:
        ops.PATH_LOG = None
    outs = [g_ for g_, u in zip(got, ups) if u is not None]
    grads = [u.to(dev()).view_as(g_) for g_, u in zip(got, ups) if u is not None]
    dh, = torch.autograd.grad(outs, hg, grads)
    torch.cuda.synchronize()
    return [g_.detach() for g_ in got], dh, log


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


NAMES = ['attn', 'q', 'a', 'z', 'theta', 'dx', 'kl']
COEF = [0.3, 0.2, 5.0, 1.0, 1.0, 1.0, 1.0]


def _upstream(got_like, present):
    ups = [COEF[i] * rnd(*g_.shape, seed=20 + i) for i, g_ in enumerate(got_like)]
    if not present:
        ups[0] = ups[1] = ups[2] = None
    return ups


def _compare_routes(tb, RP, zd, want_reg):
    from tvae import ops
    hd, E, eps_z, eps_t = _inputs(RP, zd)
    res = {}
    for present in (True, False):
        shapes = [torch.empty(B, RP)] * 3 + [torch.empty(B, zd), torch.empty(B), torch.empty(B, 2), torch.empty(B)]
        ups = _upstream(shapes, present)
        old, dh_old, log_old = _run(False, tb, hd, E, eps_z, eps_t, zd, ups)
        new, dh_new, log_new = _run(True, tb, hd, E, eps_z, eps_t, zd, ups)
        assert log_old == set()
        assert log_new == ({'head.reg'} if want_reg else set())
        assert ops.head_reg_route(RP) == want_reg
        assert bool((torch.exp(new[1][2]) == 0).any()), 'no position with expf(q) == 0: the dead branch did not run'
        for nm, o_, n_ in zip(NAMES, old, new):
            assert _same_bits(o_, n_), (nm, present)
        assert _same_bits(dh_old, dh_new), ('dheads', present)
        res[present] = (new, dh_new, ups)
    return hd, E, eps_z, eps_t, res


# (4, 5): R P = 100, most threads own nothing; (8, 17): 2 312, the 28x28 size; (8, 33): 8 712, the 64x64 size, last trip partly
# filled; (16, 24): 9 216 = NPT_MAX * 1024 exactly
@pytest.mark.parametrize('refine', [False, True])
@pytest.mark.parametrize('zd', [1, 2, 5])
@pytest.mark.parametrize('R,Ho', [(4, 5), (8, 17), (8, 33), (16, 24)])
def test_attn_head_reg(R, Ho, zd, refine):
    from tvae import ops
    from test_hip_primitives import _head_reference
    RP = R * Ho * Ho
    assert RP <= NPT_MAX * 1024
    tb = ops.HeadTables(R, Ho, SPACING, refine, math.pi, False, dev())
    hd, E, eps_z, eps_t, res = _compare_routes(tb, RP, zd, True)
    # the fp32 oracle, with all seven upstream gradients (tolerances of test_attn_head)
    got, dh, ups = res[True]
    hr = hd.clone().requires_grad_(True)
    ref = _head_reference(hr, E, eps_z, eps_t, R, Ho, zd, refine, math.pi, False, SPACING)
    for nm, r_, g_ in zip(NAMES, ref, got):
        assert rel_err(g_.reshape(-1), r_.reshape(-1)) < 5e-5, nm
    sum((r_ * u.to(r_.dtype).view_as(r_)).sum() for r_, u in zip(ref, ups)).backward()
    assert rel_err(dh, hr.grad) < 2e-4
    # float64 (tests/head_ref.py), at the same tolerances and at head_ref's own per-element / per-block budgets
    import head_ref
    f64 = head_ref.head_with_grad(hd.double().view(-1, B, RP), E, eps_z, eps_t, head_ref.tables_f64(tb), ups)
    for nm, r_, g_ in zip(NAMES, f64[0], got):
        assert rel_err(g_.reshape(-1), r_.reshape(-1)) < 5e-5, nm
    assert rel_err(dh, f64[2].reshape(dh.shape)) < 2e-4
    head_ref.assert_within(head_ref.ratios(got, dh, *f64), (R, Ho, zd, refine))


@pytest.mark.parametrize('refine', [False, True])
@pytest.mark.parametrize('zd', [1, 2, 5])
def test_attn_head_reg_boundary(zd, refine):
    """R P = 9 216 on a non-square grid takes the largest instance; 9 217 = 13 x 709 is one position too many and must run the
    strided kernels whatever the switch says (PATH_LOG, and then trivially the same bits)."""
    _compare_routes(_free_tables(9, 1024, refine), NPT_MAX * 1024, zd, True)
    _compare_routes(_free_tables(13, 709, refine), NPT_MAX * 1024 + 1, zd, False)


# ---------------------------------------------------------------------------------------------
# mid-size reductions: TVAE_MIDSIZE_ILP = 0 (one load at a time) against 1 (several in flight), bitwise
# ---------------------------------------------------------------------------------------------
def call(*a, **kw):
    from tvae._lib import call as c
    return c(*a, **kw)


def query(*a):
    from tvae._lib import query as q
    return q(*a)


def grnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator(device=dev()).manual_seed(seed), device=dev()) * scale


def _both(run):
    """run() -> list of output tensors, once per route; every output bit for bit the same."""
    res = []
    for v in ('0', '1'):
        os.environ['TVAE_MIDSIZE_ILP'] = v
        res.append([t.clone() for t in run()])
    torch.cuda.synchronize()
    for k, (o_, n_) in enumerate(zip(*res)):
        assert torch.isfinite(o_).all(), k
        assert _same_bits(o_, n_), k
    return res[1]


# slices of 16 x 8 terms: B resp. F of 1, 7, 65, 129 leave empty, partly filled and second rounds; (8, 512, 2): the bench shape
# at 8 images; (256, 512, 2): the bench shape
@pytest.mark.parametrize('B_,F_,zd', [(1, 16, 1), (7, 65, 3), (65, 7, 5), (129, 300, 2), (8, 512, 2), (256, 512, 2)])
def test_latent_bwd_ilp(B_, F_, zd):
    S, Wl, z = grnd(B_, F_, seed=1), grnd(F_, zd, seed=2), grnd(B_, zd, seed=3)

    def run():
        dWl, dz = torch.full((F_, zd), float('nan'), device=dev()), torch.full((B_, zd), float('nan'), device=dev())
        call('tvae_latent_bwd', S, Wl, z, dWl, dz, B_, F_, zd)
        return dWl, dz
    dWl, dz = _both(run)
    assert rel_err(dWl, S.double().t() @ z.double()) < 2e-5
    assert rel_err(dz, S.double() @ Wl.double()) < 2e-5


# 3 F elements six per thread and round (256 threads), images sixteen per thread and round (4 slices): F = 5 / 65 / 171 / 512 and
# B = 1 / 7 / 65 / 70 leave empty slots, partly filled rounds and second rounds; cpi 1, 2 (the unroll), 3, 7; (8, 4, 512): bench
@pytest.mark.parametrize('B_,cpi,F_', [(1, 1, 5), (7, 7, 65), (65, 3, 512), (70, 2, 171), (8, 4, 512)])
def test_dec_in_total_ilp(B_, cpi, F_):
    part0 = grnd(B_ * cpi, F_, 3, seed=1)

    def run():
        part = part0.clone()
        Simg = torch.full((B_, F_), float('nan'), device=dev())
        dbc, dWc = torch.full((F_,), float('nan'), device=dev()), torch.full((F_, 2), float('nan'), device=dev())
        call('tvae_dec_in_total', part, B_, cpi, F_, Simg, dbc, dWc)
        return Simg, dbc, dWc
    Simg, dbc, dWc = _both(run)
    p64 = part0.double().view(B_, cpi, F_, 3)
    assert rel_err(Simg, p64[..., 0].sum(1)) < 2e-5
    assert rel_err(dbc, p64[..., 0].sum((0, 1))) < 2e-5
    assert rel_err(dWc, p64[..., 1:].sum((0, 1))) < 2e-5


# panels of 512 columns in 64 groups: 300 -> 5 per group (pairs + one, last group 5 of 5 ... a short one), 707 -> 12 per group
# (eight at once, two pairs; the last group 11: eight, a pair, one), 1153 -> 19 (two eights, a pair, one)
@pytest.mark.parametrize('npan', [300, 707, 1153])
def test_heads_bwd_totals_ilp(npan):
    nh, C, act = 3, 32, 1
    N = npan * 512 - 37
    W, dY, X = grnd(nh, C, seed=1, scale=C ** -0.5), grnd(nh, N, seed=2), grnd(C, N, seed=3).clamp(-0.9, 0.9)
    used = npan * C * (nh + 1)
    part = torch.empty(((used + 3) & ~3) + 64 * C * (nh + 1), device=dev())      # room for the 64 group partials: two stages

    def run():
        tot = torch.full((nh + 1, C), float('nan'), device=dev())
        call('tvae_heads_bwd', W, dY, N, X, N, None, N, nh, C, N, act, 0.01, part, part.numel(), tot)
        return tot,
    tot, = _both(run)
    dpre = (W.double().t() @ dY.double()) * torch.where(X.double() > 0, 1.0, 0.01)
    assert rel_err(tot[nh], dpre.sum(1)) < 1e-4          # (sums of up to 590 000 fp32 terms)
    assert rel_err(tot[:nh], dY.double() @ X.double().t()) < 1e-4


# slabs = chunks of 32 columns, one per workgroup up to the number of CUs: 1, 7 and 65 slabs, and 8 images of the bench shape
# (8 x 8 x 33^2 columns rounded down to whole chunks: 256 slabs)
@pytest.mark.parametrize('N', [32, 7 * 32, 65 * 32, 8 * 8 * 33 * 33 // 32 * 32])
def test_enc_tail_wgrad_total_ilp(N):
    C, rows_d = 128, 5
    D, A = grnd(rows_d, N, seed=1), grnd(C, N, seed=2)
    amax_d = (8.0 * D.abs().max()).reshape(1)
    amax_a = (8.0 * A.abs().amax(dim=1)).contiguous()
    ws = torch.empty(query('tvae_enc_tail_wgrad_x6_ws_floats', N), device=dev())

    def run():
        out = torch.full((C, C), float('nan'), device=dev())
        call('tvae_enc_tail_wgrad_wide', D, N, rows_d, A, N, out, ws, ws.numel(), C, N, amax_d, amax_a)
        return out[:rows_d],
    got, = _both(run)
    assert rel_err(got, D.double() @ A.double().t()) < 1e-4


# columns (image, row) 256 per round of a workgroup, eight rounds in flight: 3 x 33 = 99 (most threads own nothing), 8 x 33 = 264
# (a second, nearly empty column per thread; the bench shape at 8 images)
@pytest.mark.parametrize('B_', [3, 8])
def test_dft_dbias_ilp(B_):
    Cin, n, k, pad, C, R = 1, 64, 64, 16, 32, 8
    Ho = n + 2 * pad - k + 1
    y, bank, bias = grnd(B_, Cin, n, n, seed=1), grnd(C * R, k * k, seed=2, scale=0.02), grnd(C, seed=3)
    at = torch.zeros(query('tvae_conv1_dft_at_floats', B_, Cin, n, k, pad, C, R), device=dev())
    wsd = torch.empty(query('tvae_conv1_dft_ws_floats', B_, Cin, n, k, pad, C, R), device=dev())
    out = torch.empty(C, B_ * R * Ho * Ho, device=dev())
    call('tvae_conv1_fwd_dft', y, bank, bias, out, at, wsd, wsd.numel(), B_, Cin, n, k, pad, C, R, 0, 0.01, 3)
    gg = grnd(C, B_ * R * Ho * Ho, seed=4)

    def run():
        dbank, dbias = torch.full((C * R, k * k), float('nan'), device=dev()), torch.full((C,), float('nan'), device=dev())
        call('tvae_conv1_wgrad_dft', gg, at, dbank, dbias, wsd, wsd.numel(), B_, Cin, n, k, pad, C, R, 3)
        return dbias, dbank
    dbias, _ = _both(run)
    assert rel_err(dbias, gg.double().sum(1)) < 2e-5
