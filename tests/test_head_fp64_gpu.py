"""Attention head (tvae_attn_head_fwd / _bwd: register-resident, strided and chunked kernels of csrc/small_kernels.hpp) against
tests/head_ref.py, the float64 restatement -- every route of csrc/abi_small.hip (head_reg_npt, head_chunks), nothing compared at
whole-tensor granularity:

  attn, q      per element, absolute              a     per element, relative (reference >= 2^-100; below: |got| <= 2^-99)
  z, theta, dx, kl   per image and component      dheads   per (head row, image) block, relative to the block's own maximum

each against K u (condition quantity), u = 2^-24; the condition quantities are derived in head_ref's docstring.  K: fp32 on the
CPU (the oracle's posterior_pool_kl and its autograd) against head_ref on these inputs, 8 x the worst ratio and not below 16
(tests/test_head_ref_cpu.py::test_budget_constants measures and prints them; never against the kernels):

    quantity   attn   q      a      z      theta  dx     kl     dheads
    ratio      1.00   1.00   0.47   0.09   0.75   0.17   0.19   0.17
    K          16     16     16     16     16     16     16     16

Inputs: test_midsize_kernels._inputs (E at 1e-30 and 1 - 2^-24, an image shifted by -200, an image with every other logit
shifted by -200: positions with expf(q) == 0, asserted present) and the same with the logits x 30 (peaked).  All seven upstream
gradients at coefficient 1, and only the four of the training step.  Routes that the code states to be bit-identical (register
against strided, ILP on / off) keep their bitwise tests in test_midsize_kernels.py."""
import math
import os

import pytest
import torch

import guardband
import head_ref

pytestmark = pytest.mark.gpu
SPACING = 2.0 / 27
REG_MAX = 9 * 1024


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in test_hip_primitives.py: every C-ABI call on relocated tensors between guard bands, twice from the same inputs."""
    with guardband.GuardedCalls(replay=True):
        yield


@pytest.fixture(autouse=True)
def restore_switch():
    old = os.environ.get('TVAE_HEAD_REG')
    yield
    if old is None:
        os.environ.pop('TVAE_HEAD_REG', None)
    else:
        os.environ['TVAE_HEAD_REG'] = old


def dev():
    return torch.device('cuda:0')


def call(*a, **kw):
    from tvae._lib import call as c
    return c(*a, **kw)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def chunks(B, RP, zd):
    """head_chunks of csrc/abi_small.hip with the scratch of ops.HeadFn (never the limit): workgroups per image."""
    if B >= 128 or RP < 16384 or zd > 64:
        return 1
    G = min((RP + 4095) // 4096, 1024 // B)
    if G < 2:
        return 1
    chunk = (RP + G - 1) // G
    return (RP + chunk - 1) // chunk


def part_floats(zd):
    return 4 + 3 + 3 * (zd + 1)                          # (small_kernels.hpp: head_part_floats)


def tables(R, P, refine):
    """ops.HeadTables where P is a square grid, else the free tables of test_midsize_kernels (random, normalised priors)."""
    from tvae import ops
    from test_midsize_kernels import _free_tables
    Ho = math.isqrt(P)
    return ops.HeadTables(R, Ho, SPACING, refine, math.pi, False, dev()) if Ho * Ho == P else _free_tables(R, P, refine)


def inputs(B, RP, zd, peaked):
    """B = 3: head_ref.case_inputs.  Other B: the same construction -- image 0 with the two extreme E, image 1 (B > 2) shifted by
    -200 as a whole, the last image with every other logit shifted by -200."""
    if B == 3:
        return head_ref.case_inputs(RP, zd, peaked)
    hd = rnd(3 + 2 * zd, B * RP, seed=1, scale=0.5)
    hd[0] *= 30.0 if peaked else 4.0
    if B > 2:
        hd[0, RP:2 * RP] -= 200.0
    hd[0, (B - 1) * RP + 1:B * RP:2] -= 200.0
    E = torch.empty(B, RP).exponential_(generator=torch.Generator().manual_seed(2))
    E[0, 0] = 1e-30
    E[0, RP - 1] = 1.0 - 2.0 ** -24
    return hd, E, rnd(B, zd, seed=3), rnd(B, seed=4)


def run_fn(tb, hd, E, eps_z, eps_t, B, zd, ups):
    """Through ops.HeadFn.  -> (outputs, dheads, floats of the chunk scratch written by the forward, by the backward)"""
    from tvae import ops
    part = ops._scratch(dev(), 'head_part', 1024 * (7 + 3 * (zd + 1)))
    hg = hd.clone().to(dev()).requires_grad_(True)
    part.fill_(float('nan'))
    got = ops.HeadFn.apply(hg, E.to(dev()), eps_z.to(dev()), eps_t.to(dev()), tb, B, zd)
    wrote_f = int((~torch.isnan(part)).sum())
    part.fill_(float('nan'))
    outs = [g_ for g_, u_ in zip(got, ups) if u_ is not None]
    grads = [u_.to(dev()).view_as(g_) for g_, u_ in zip(got, ups) if u_ is not None]
    dh, = torch.autograd.grad(outs, hg, grads)
    wrote_b = int((~torch.isnan(part)).sum())
    torch.cuda.synchronize()
    return [g_.detach() for g_ in got], dh, wrote_f, wrote_b


def run_abi(tb, hd, E, eps_z, eps_t, B, zd, ups, pad=0, part=None, part_b=None):
    """Through the C ABI: row stride B R P + pad (pad columns of heads hold 1e30, those of dheads have to stay as they were);
    part / part_b: the chunk scratch of the forward / backward, None for NULL.  -> (outputs, dheads [nh][B R P])"""
    nh, RP = 3 + 2 * zd, tb.R * tb.P
    N, ldh = B * RP, B * RP + pad
    heads = torch.full((nh, ldh), 1e30)
    heads[:, :N] = hd
    heads = heads.to(dev())
    e, ez, et = E.to(dev()), eps_z.to(dev()), eps_t.to(dev())
    new = lambda *s: torch.full(s, float('nan'), device=dev())
    attn, q, a, z, th, dx, kl = new(B, RP), new(B, RP), new(B, RP), new(B, zd), new(B), new(B, 2), new(B)
    call('tvae_attn_head_fwd', heads, ldh, e, ez, et, tb.p_r, tb.off, tb.p_tr, tb.grid, B, tb.R, tb.P, zd, tb.sigma_p,
         tb.theta_off_scale, attn, q, a, z, th, dx, kl, part, 0 if part is None else part.numel())
    g = [None if u_ is None else u_.to(dev()).contiguous() for u_ in ups]
    dheads = torch.full((nh, ldh), -7.0, device=dev())
    call('tvae_attn_head_bwd', heads, ldh, q, a, ez, et, tb.p_r, tb.off, tb.p_tr, tb.grid, B, tb.R, tb.P, zd, tb.sigma_p,
         tb.theta_off_scale, g[3], g[4], g[5], g[6], g[0], g[1], g[2], dheads, part_b, 0 if part_b is None else part_b.numel())
    torch.cuda.synchronize()
    assert bool((dheads[:, N:] == -7.0).all()), 'the pad columns of dheads were written'
    return [attn, q, a, z, th, dx, kl], dheads[:, :N].contiguous()


def check(got, dh, hd, E, eps_z, eps_t, tb, B, ups, what):
    RP = tb.R * tb.P
    ref = head_ref.head_with_grad(hd.double().view(-1, B, RP), E, eps_z, eps_t, head_ref.tables_f64(tb), ups)
    r = head_ref.ratios(got, dh, *ref)
    print(what, {k_: round(v, 3) for k_, v in r.items() if k_ != 'dheads_blocks'})
    if r['dheads'] > head_ref.K['dheads']:
        row, img = divmod(int(r['dheads_blocks'].argmax()), B)
        what = (what, 'worst dheads block: row %d image %d' % (row, img))
    head_ref.assert_within(r, what)


def sweep(R, P, zd, B=3, want_reg=None, want_G=1, variants=((False, False), (False, True), (True, True))):
    """One shape through ops.HeadFn: (peaked, refine) variants x (seven, four) upstream gradients; the route is asserted from
    PATH_LOG (register) and from what the launches wrote to the chunk scratch (G workgroups per image)."""
    from tvae import ops
    RP = R * P
    for peaked, refine in variants:
        tb = tables(R, P, refine)
        hd, E, eps_z, eps_t = inputs(B, RP, zd, peaked)
        for seven in (True, False):
            ups = head_ref.upstream(B, RP, zd, seven)
            ops.PATH_LOG = set()
            try:
                got, dh, wf, wb = run_fn(tb, hd, E, eps_z, eps_t, B, zd, ups)
                log = ops.PATH_LOG
            finally:
                ops.PATH_LOG = None
            if want_reg is not None:
                assert (log == {'head.reg'}) == want_reg and ops.head_reg_route(RP) == want_reg
            assert chunks(B, RP, zd) == want_G
            assert (wf, wb) == ((B * want_G * part_floats(zd), B * want_G * 2) if want_G > 1 else (0, 0)), (wf, wb, want_G)
            assert bool((torch.exp(got[1]) == 0).any()), 'no position with expf(q) == 0: the dead branch did not run'
            check(got, dh, hd, E, eps_z, eps_t, tb, B, ups, (R, P, zd, B, peaked, refine, seven))


# R P = 100 (most threads own nothing), 2 312, 8 712 (last trip partly filled), 9 216 = 9 x 1024: the four register instances, and
# the strided kernels at the same sizes (TVAE_HEAD_REG=0)
@pytest.mark.parametrize('reg', [True, False])
@pytest.mark.parametrize('zd', [1, 2, 5, 9])
@pytest.mark.parametrize('R,Ho', [(4, 5), (8, 17), (8, 33), (16, 24)])
def test_head_one_workgroup_per_image(R, Ho, zd, reg):
    os.environ['TVAE_HEAD_REG'] = '1' if reg else '0'
    sweep(R, Ho * Ho, zd, want_reg=reg)


# 9 217 = 13 x 709: one position too many for the register kernels, whatever the switch says
@pytest.mark.parametrize('zd', [2, 5])
def test_head_strided_beyond_the_register_sizes(zd):
    os.environ['TVAE_HEAD_REG'] = '1'
    sweep(13, 709, zd, want_reg=False)


# 16 384 = 4 x 64^2: the first chunked size (4 workgroups per image); 16 383 = 3 x 5461 must not chunk; 34 848 = 8 x 66^2: 9
@pytest.mark.parametrize('zd', [1, 2, 5, 9])
@pytest.mark.parametrize('R,P,G', [(4, 64 * 64, 4), (3, 5461, 1), (8, 66 * 66, 9)])
def test_head_chunked(R, P, G, zd):
    sweep(R, P, zd, want_G=G, variants=((False, False), (True, True)))


# B = 127: 1024 / B = 8 workgroups per image where the size asks for 9 (the cap); B = 128: one workgroup per image again
@pytest.mark.parametrize('B,R,P,G', [(127, 8, 66 * 66, 8), (128, 4, 64 * 64, 1)])
def test_head_chunk_cap_and_many_images(B, R, P, G):
    sweep(R, P, 1, B=B, want_G=G, variants=((False, True),))


# z_dim 50 (the galaxy value: ragged groups of HEAD_CG = 4 and of HEAD_BD = 8), 64 (the last chunked one: tot[3 + 3 * 65] full),
# 65 (must take the unchunked kernels), at B = 2, R P = 16 384
@pytest.mark.parametrize('zd,G', [(50, 4), (64, 4), (65, 1)])
def test_head_chunked_wide_latent(zd, G):
    sweep(4, 64 * 64, zd, B=2, want_G=G, variants=((False, True),))


# row stride B R P + 37, the pad columns of heads at 1e30 and those of dheads left alone: a register and a chunked case
@pytest.mark.parametrize('R,Ho,zd', [(8, 17, 2), (4, 64, 5)])
def test_head_padded_row_stride(R, Ho, zd):
    B, RP = 3, R * Ho * Ho
    tb = tables(R, Ho * Ho, True)
    hd, E, eps_z, eps_t = inputs(B, RP, zd, False)
    G = chunks(B, RP, zd)
    for seven in (True, False):
        ups = head_ref.upstream(B, RP, zd, seven)
        part = torch.full((1024 * (7 + 3 * (zd + 1)),), float('nan'), device=dev())
        part_b = part.clone()
        got, dh = run_abi(tb, hd, E, eps_z, eps_t, B, zd, ups, pad=37, part=part, part_b=part_b)
        assert int((~torch.isnan(part)).sum()) == (B * G * part_floats(zd) if G > 1 else 0)
        assert int((~torch.isnan(part_b)).sum()) == (B * G * 2 if G > 1 else 0)
        check(got, dh, hd, E, eps_z, eps_t, tb, B, ups, (R, Ho, zd, 'ldh + 37', seven))


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def test_head_chunk_scratch_missing_or_short():
    """part = NULL, and a part one float short of what the chunked kernels need (forward: B G head_part_floats, backward: 2 B G),
    at a chunked size: the one-workgroup-per-image kernels run, the two give the same bits, the short scratch stays unwritten,
    and the result meets the float64 reference like every other route."""
    B, R, Ho, zd = 3, 4, 64, 2
    RP = R * Ho * Ho
    G = chunks(B, RP, zd)
    assert G == 4
    tb = tables(R, Ho * Ho, True)
    hd, E, eps_z, eps_t = inputs(B, RP, zd, False)
    ups = head_ref.upstream(B, RP, zd, True)
    none, dh_none = run_abi(tb, hd, E, eps_z, eps_t, B, zd, ups)
    part = torch.full((B * G * part_floats(zd) - 1,), float('nan'), device=dev())
    part_b = torch.full((B * G * 2 - 1,), float('nan'), device=dev())
    short, dh_short = run_abi(tb, hd, E, eps_z, eps_t, B, zd, ups, part=part, part_b=part_b)
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(part_b).all())
    for nm, x, y in zip(head_ref.NAMES + ['dheads'], none + [dh_none], short + [dh_short]):
        assert _same_bits(x, y), nm
    check(none, dh_none, hd, E, eps_z, eps_t, tb, B, ups, 'part = NULL')
    # (and with the scratch exactly large enough the chunked kernels do run)
    part = torch.full((B * G * part_floats(zd),), float('nan'), device=dev())
    part_b = torch.full((B * G * 2,), float('nan'), device=dev())
    full, dh_full = run_abi(tb, hd, E, eps_z, eps_t, B, zd, ups, part=part, part_b=part_b)
    assert not bool(torch.isnan(part).any()) and not bool(torch.isnan(part_b).any())
    check(full, dh_full, hd, E, eps_z, eps_t, tb, B, ups, 'part exactly large enough')
