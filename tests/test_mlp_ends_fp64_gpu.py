"""The streaming kernels at the two ends of the MLPs through their C-ABI entry points -- tvae_rowdot_seg, tvae_seg_sum,
tvae_coldot, tvae_outer_mask, tvae_act_bwd, tvae_dec_l0_fwd, tvae_latent_bias, tvae_latent_bwd, tvae_fourier_fwd / _bwd,
tvae_dec_out_bwd, tvae_dec_in_bwd, tvae_heads_fwd / _bwd -- against tests/mlp_ends_ref.py in float64, one case for every branch
(case lists and what each reaches: mlp_ends_ref.py; tests/test_mlp_ends_ref_cpu.py checks the branch arithmetic of the lists).

EVERY element of every output against K u (condition quantity), u = 2^-24 (K and the condition quantities: mlp_ends_ref's
docstring; K comes from fp32 CPU arithmetic, never from these kernels).  Strided inputs carry 1e30 in their pad columns,
strided outputs are prefilled with a sentinel that has to come back untouched; amax, refusals and the totals with and without
the optional stores are exact.  Every call runs between guard bands, twice (replay).

Worst ratio seen on an MI355X, by output: mlp_ends_ref.GPU_SEEN; test_worst_ratios prints this run's.

One-line changes to the kernels that test_hip_primitives.py and test_midsize_kernels.py pass and this file fails (each run
once): rowdot_seg_kernel without its trailing `if (i < n4)` float4; fourier_bwd_kernel staging every chunk's weights from
f = threadIdx.x; load4 returning x = 0 in the element-wise tail of the VECTORISED instance (w = 0 there is no change at all: the
tail is only entered when w is out of range, and the scalar instance's w the earlier tests catch too); act_deriv_from_out with
y >= 0 (the earlier files notice it only through exact zeros that happen to be among millions of normal draws)."""
import math

import pytest
import torch

import guardband
import mlp_ends_ref as R

pytestmark = pytest.mark.gpu
WORST = {}
NAN = float('nan')


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in test_hip_primitives.py: every C-ABI call on relocated tensors between guard bands, twice from the same inputs."""
    with guardband.GuardedCalls(replay=True):
        yield


def dev():
    return torch.device('cuda:0')


def call(*a, **kw):
    from tvae._lib import call as c
    return c(*a, **kw)


def G(t):
    return None if t is None else t.contiguous().to(dev())


def strided(T, ld, fill=R.PAD_IN):
    """T [rows][N] as the leading columns of a [rows][ld] device tensor whose pad columns hold `fill`."""
    out = torch.full((T.shape[0], ld), fill)
    out[:, :T.shape[1]] = T
    return out.to(dev())


def full(shape, v=R.SENTINEL):
    return torch.full(shape, v, device=dev())


def check(name, got, ref, cond, floor=None, what=None):
    r = R.ratio(got, ref, cond, floor)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f'{name} {"" if what is None else what}: ratio {r:.3f} of K = {R.K[name]}')
    assert math.isfinite(r) and r <= R.K[name], (name, what, r, R.K[name])


def pads_untouched(T, N):
    assert bool((T[:, N:] == R.SENTINEL).all()), 'pad columns of a strided output were written'


# ---- tvae_rowdot_seg --------------------------------------------------------------------------------------------------------
def rowsum_arg(X, layout):
    """-> (the tensor to pass, ldx): X [M][N] inside a flat buffer of pad values."""
    M, N = X.shape
    ldx = R.ld_pad4(N) + (layout == 'ldx1')
    off = int(layout == 'view')
    buf = torch.full((M * ldx + off,), R.PAD_IN)
    buf[off:].view(M, ldx)[:, :N] = X
    arg = buf.to(dev())[off:]
    assert arg.data_ptr() % 16 == 4 * off and arg.is_contiguous()
    return arg, ldx


@pytest.mark.parametrize('shape,layout', R.ROWSUM_CASES)
def test_rowsum_forms(shape, layout):
    """Plain row sums (V == NULL): the 16-byte form -- paired loads, one trailing float4, dword tail -- and the dword form the same
    data takes from a misaligned X, from ldx = 4 k + 1 and in segments that begin at a column that is no multiple of 4."""
    seglen, N = shape
    X = R.rowsum_case(seglen, N)
    arg, ldx = rowsum_arg(X, layout)
    nseg = (N + seglen - 1) // seglen
    form16 = [layout == 'aligned' and (s * seglen) % 4 == 0 for s in range(nseg)]
    if seglen == 3151:
        assert form16 == ([True, False, False, False, True] if layout == 'aligned' else [False] * 5)
    else:
        assert all(form16) == (layout == 'aligned')
    out = full((nseg, R.ROWSUM_M))
    amax = torch.zeros(1, device=dev())
    call('tvae_rowdot_seg', arg, ldx, None, 1, R.ROWSUM_M, N, seglen, out, amax)
    ref, cond = R.rowsum_ref(seglen, N)
    check('rowdot', out, ref, cond, what=(shape, layout))
    assert float(amax) == float(X.abs().max())


@pytest.mark.parametrize('no', R.ROWDOT_V_CASES)
def test_rowdot_with_v(no):
    X, V = R.rowdot_v_case(no)
    M, N = X.shape
    out = full((3, M, no))
    call('tvae_rowdot_seg', G(X), N, G(V), no, M, N, 500, out, None)
    check('rowdot', out, *R.both(R.rowdot_seg, X, V, 500), what=('V', no))


@pytest.mark.parametrize('where', list(R.AMAX_PLANTS))
def test_rowsum_amax_planted(where):
    """The largest |x| is negative and met by one particular load of one form: amax has to equal it exactly."""
    seglen, N = 3151, 13381
    X = R.rowsum_case(seglen, N).clone()
    r, c = R.AMAX_PLANTS[where]
    X[r, c] = -77.5
    assert float(X.abs().max()) == 77.5 and float(X.max()) < 10
    arg, ldx = rowsum_arg(X, 'aligned')
    out, amax = full((5, R.ROWSUM_M)), torch.zeros(1, device=dev())
    call('tvae_rowdot_seg', arg, ldx, None, 1, R.ROWSUM_M, N, seglen, out, amax)
    assert float(amax) == 77.5
    check('rowdot', out, *R.both(R.rowdot_seg, X, None, seglen), what=('amax', where))


def test_rowsum_amax_keeps_a_larger_value_and_refusals():
    seglen, N = 1600, 2601
    X = R.rowsum_case(seglen, N)
    arg, ldx = rowsum_arg(X, 'aligned')
    out, amax = full((2, R.ROWSUM_M)), torch.full((1,), 1000.0, device=dev())
    call('tvae_rowdot_seg', arg, ldx, None, 1, R.ROWSUM_M, N, seglen, out, amax)
    assert float(amax) == 1000.0
    check('rowdot', out, *R.rowsum_ref(seglen, N), what='preloaded amax')
    Xv, V = R.rowdot_v_case(4)
    V5 = torch.cat([V, V[:, :1]], 1)
    out, amax = full((3, 37, 5)), torch.full((1,), 0.5, device=dev())
    with pytest.raises(Exception):
        call('tvae_rowdot_seg', G(Xv), 1203, G(V5), 5, 37, 1203, 500, out, amax)
    with pytest.raises(Exception):
        call('tvae_rowdot_seg', G(Xv), 1203, G(V), 4, 37, 1203, 0, out, amax)
    assert bool((out == R.SENTINEL).all()) and float(amax) == 0.5


# ---- tvae_seg_sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,L', R.SEG_SUM_CASES)
def test_seg_sum_boundaries(S, L):
    X, out0 = R.seg_sum_case(S, L)
    Xd = G(X)
    for scale, acc in R.SEG_SUM_MODES:
        out = G(out0).clone()
        call('tvae_seg_sum', Xd, S, L, out, scale, acc)
        check('seg_sum', out, *R.both(R.seg_sum, X, out0, scale, acc), what=(S, L, scale, acc))


# ---- tvae_coldot / tvae_outer_mask / tvae_act_bwd ---------------------------------------------------------------------------
@pytest.mark.parametrize('no,lay,act,has_b', R.SKINNY_CASES)
def test_skinny_products_and_masks(no, lay, act, has_b):
    M, N = R.SKINNY_M, R.SKINNY_N
    H, W, b, dy = R.skinny_case(no, act)
    Wd, wsm, wso = (G(W), 1, M) if lay == 0 else (G(W.t()), no, 1)
    ldh, ldd = N + 4, N + 8
    Hs = strided(H, ldh)
    out = full((N, no), NAN)
    call('tvae_coldot', Hs, ldh, M, N, Wd, wsm, wso, G(b) if has_b else None, no, out)
    check('coldot', out, *R.both(R.coldot, H, W, b if has_b else None), what=(no, lay, has_b))
    D = full((M, ldd))
    call('tvae_outer_mask', G(dy), no, Wd, wsm, wso, Hs, ldh, D, ldd, M, N, act, 0.01)
    check('outer_mask', D[:, :N], *R.both(R.outer_mask, dy, W, H, act), what=(no, lay, act))
    pads_untouched(D, N)
    dY = R.rnd(M, N, seed=5)
    dpre = full((M, N), NAN)
    call('tvae_act_bwd', G(dY), G(H), dpre, M * N, act, 0.01)
    check('act_bwd', dpre, *R.both(R.act_bwd, dY, H, act), what=('act', act))


def test_skinny_products_refuse_five_outputs():
    H, W, b, dy = R.skinny_case(4, 2)
    M, N = H.shape
    out, D = full((N, 5)), full((M, N))
    with pytest.raises(Exception):
        call('tvae_coldot', G(H), N, M, N, G(torch.cat([W, W[:1]])), 1, M, None, 5, out)
    with pytest.raises(Exception):
        call('tvae_outer_mask', G(torch.cat([dy, dy[:, :1]], 1)), 5, G(torch.cat([W, W[:1]])), 1, M, G(H), N, D, N, M, N, 2, 0.01)
    assert bool((out == R.SENTINEL).all()) and bool((D == R.SENTINEL).all())


# ---- tvae_dec_l0_fwd / tvae_latent_bias / tvae_latent_bwd -------------------------------------------------------------------
@pytest.mark.parametrize('F,zd,act,has_lb', R.L0_CASES)
def test_first_layer_forward(F, zd, act, has_lb):
    B, Np = R.L0_B, R.L0_NP
    Nt, ldh = B * Np, B * Np + 4
    xr, Wc, bc, Wl, z = R.l0_case(F, zd)
    LB = full((B, F), NAN)
    call('tvae_latent_bias', G(Wl), G(z), LB, B, F, zd)
    check('latent_bias', LB, *R.both(R.latent_bias, Wl, z), what=(F, zd))
    lb = R.latent_bias(Wl, z).float() if has_lb else None      # (the reference's LB rounded once: the layer is checked on its own)
    h = full((F, ldh))
    call('tvae_dec_l0_fwd', G(xr), G(Wc), G(bc), G(lb), h, ldh, F, Nt, Np, act, 0.01)
    check('dec_l0', h[:, :Nt], *R.both(R.dec_l0_fwd, xr, Wc, bc, lb, Np, act), what=(F, act, has_lb))
    pads_untouched(h, Nt)


@pytest.mark.parametrize('B,F,zd', R.LATENT_BWD_CASES)
def test_latent_bwd(B, F, zd):
    S, Wl, z = R.latent_bwd_case(B, F, zd)
    dWl, dz = full((F, zd), NAN), full((B, zd), NAN)
    call('tvae_latent_bwd', G(S), G(Wl), G(z), dWl, dz, B, F, zd)
    ref, cond = R.both(R.latent_bwd, S, Wl, z)
    check('dWl', dWl, ref['dWl'], cond['dWl'], what=(B, F, zd))
    check('dz', dz, ref['dz'], cond['dz'], what=(B, F, zd))


# ---- tvae_fourier_fwd / _bwd ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,sigma', R.FOURIER_FWD_CASES)
def test_fourier_fwd(F, sigma):
    Nt, ld = R.FOURIER_NT, R.FOURIER_NT + 4
    xr, Wf, bf, _ = R.fourier_case(F)
    feat = full((F, ld))
    call('tvae_fourier_fwd', G(xr), G(Wf), G(bf), sigma, feat, ld, F, Nt)
    check('fourier_fwd', feat[:, :Nt], *R.both(R.fourier_fwd, xr, Wf, bf, sigma), what=(F, sigma))
    pads_untouched(feat, Nt)


@pytest.mark.parametrize('F,sigma', R.FOURIER_BWD_CASES)
def test_fourier_bwd(F, sigma):
    """Features in LDS chunks of 256: one partly filled chunk, exactly one, one and a single feature, one and 44, four."""
    Nt, ld = R.FOURIER_NT, R.FOURIER_NT + 4
    xr, Wf, bf, g = R.fourier_case(F)
    gx = full((Nt, 2), NAN)
    call('tvae_fourier_bwd', G(xr), G(Wf), G(bf), sigma, strided(g, ld), ld, F, Nt, gx)
    ref, cond = R.both(R.fourier_bwd, xr, Wf, bf, sigma, g)
    floor = R.fourier_bwd_floor(xr, Wf, bf, sigma, g)
    err = (gx.double().cpu() - ref).abs()
    share = float((err - R.K['fourier_bwd'] * R.U * cond).div(floor).max())          # > 0: the floor was drawn on
    bare = R.ratio(gx, ref, cond)
    WORST['fourier_bwd floor share'] = max(WORST.get('fourier_bwd floor share', -math.inf), share)
    WORST['fourier_bwd without floor'] = max(WORST.get('fourier_bwd without floor', 0.0), bare)
    print(f'fourier_bwd {(F, sigma)}: (error - K u cond) / floor = {share:.3f} at most; error without the floor: {bare:.2f} u cond')
    check('fourier_bwd', gx, ref, cond, floor, what=(F, sigma))


# ---- tvae_dec_out_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,N,ldh,ldd,no,act', R.DEC_OUT_CASES)
def test_dec_out_bwd(F, N, ldh, ldd, no, act):
    gy, Wo, H = R.dec_out_case(F, N, no, act)
    npan = (N + 1023) // 1024
    Hs, gyd, Wod = strided(H, ldh), G(gy), G(Wo)
    D, tot = full((F, ldd)), full((1 + no, F), NAN)
    part = torch.zeros(npan * F * (1 + no), device=dev())
    call('tvae_dec_out_bwd', gyd, no, Wod, Hs, ldh, D, ldd, F, N, act, 0.01, part, part.numel(), tot)
    ref, cond = R.dec_out_ref(F, N, no, act)
    check('out_D', D[:, :N], ref['out_D'], cond['out_D'], what=(F, N))
    pads_untouched(D, N)
    check('out_tot', tot, ref['out_tot'], cond['out_tot'], what=(F, N))
    tot2 = full((1 + no, F), NAN)                              # D == NULL: the totals alone, bit for bit those of the run with D
    call('tvae_dec_out_bwd', gyd, no, Wod, Hs, ldh, None, ldd, F, N, act, 0.01, part.zero_(), part.numel(), tot2)
    assert torch.equal(tot2, tot)


def test_dec_out_and_dec_in_refusals():
    F, N, ldh, ldd, no, act = R.DEC_OUT_CASES[3]
    gy, Wo, H = R.dec_out_case(F, N, no, act)
    need = 2 * F * (1 + no)
    D, tot, part = full((F, ldd)), full((1 + no, F)), full((need,))
    with pytest.raises(Exception):
        call('tvae_dec_out_bwd', G(gy), no, G(Wo), strided(H, ldh), ldh, D, ldd, F, N, act, 0.01, part, need - 1, tot)
    gy5, Wo5 = torch.cat([gy] * 5, 1), torch.cat([Wo] * 5)
    big = full((2 * F * 6,))
    with pytest.raises(Exception):
        call('tvae_dec_out_bwd', G(gy5), 5, G(Wo5), strided(H, ldh), ldh, D, ldd, F, N, act, 0.01, big, big.numel(), tot)
    for t in (D, tot, part, big):
        assert bool((t == R.SENTINEL).all())
    F, B, Np, ldd = R.DEC_IN_CASES[2]
    d, xr, Wc = R.dec_in_case(F, B, Np)
    need = B * 2 * F * 3
    outs = [full((B * Np, 2)), full((B, F)), full((F,)), full((F, 2)), full((need,))]
    with pytest.raises(Exception):
        call('tvae_dec_in_bwd', strided(d, ldd), ldd, G(xr), G(Wc), F, B, Np, *outs, need - 1)
    for t in outs:
        assert bool((t == R.SENTINEL).all())


# ---- tvae_dec_in_bwd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,B,Np,ldd', R.DEC_IN_CASES)
def test_dec_in_bwd(F, B, Np, ldd):
    """Simg per image and feature: a panel that read into the next image would show there (and in gxr of that image)."""
    d, xr, Wc = R.dec_in_case(F, B, Np)
    Nt, cpi = B * Np, (Np + 1023) // 1024
    gxr, Simg, dbc, dWc = full((Nt, 2), NAN), full((B, F), NAN), full((F,), NAN), full((F, 2), NAN)
    part = torch.zeros(B * cpi * F * 3, device=dev())
    call('tvae_dec_in_bwd', strided(d, ldd), ldd, G(xr), G(Wc), F, B, Np, gxr, Simg, dbc, dWc, part, part.numel())
    ref, cond = R.both(R.dec_in_bwd, d, xr, Wc, B, Np)
    for n_, got in (('in_gxr', gxr), ('in_Simg', Simg), ('in_dbc', dbc), ('in_dWc', dWc)):
        check(n_, got, ref[n_], cond[n_], what=(F, B, Np))


# ---- tvae_heads_fwd / _bwd --------------------------------------------------------------------------------------------------
def run_heads(nh, C, N, ldx, ldy, act, has_b, extra_ws):
    W, b, X, dY = R.heads_case(nh, C, N, act)
    Wd, Xs = G(W), strided(X, ldx)
    Y = full((nh, ldy))
    call('tvae_heads_fwd', Wd, Xs, ldx, G(b) if has_b else None, Y, ldy, nh, C, N)
    check('heads_Y', Y[:, :N], *R.both(R.heads_fwd, W, X, b if has_b else None), what=(nh, C, N, ldx))
    pads_untouched(Y, N)
    ref, cond = R.heads_ref(nh, C, N, act)
    npan, dYs = (N + 511) // 512, strided(dY, ldy)
    tots = []
    for ws_floats in extra_ws:
        for with_dx in (True, False):
            dX, tot = full((C, ldy)), full((nh + 1, C), NAN)
            part = torch.zeros(npan * C * (nh + 1) + ws_floats, device=dev())
            call('tvae_heads_bwd', Wd, dYs, ldy, Xs, ldx, dX if with_dx else None, ldy, nh, C, N, act, 0.01, part, part.numel(), tot)
            if with_dx:
                check('heads_dX', dX[:, :N], ref['heads_dX'], cond['heads_dX'], what=(nh, C, N, ldx, act))
                pads_untouched(dX, N)
                check('heads_tot', tot, ref['heads_tot'], cond['heads_tot'], what=(nh, C, N, ldx, act, ws_floats))
                tots.append(tot)
            else:
                assert torch.equal(tot, tots[-1])            # dX == NULL: the same sums, bit for bit
    return tots


@pytest.mark.parametrize('nh,C,lay,act,has_b', R.HEADS_CASES)
def test_heads(nh, C, lay, act, has_b):
    run_heads(nh, C, lay[0], lay[1], lay[2], act, has_b, [0])


def test_heads_both_total_routes():
    """256 panels: the single-stage totals with exactly np C (nh + 1) floats of workspace, the two coalesced stages with room for
    the 64 group partials behind them.  Both meet the float64 bound; they need not agree in bits."""
    nh, C, N, act = R.HEADS_BIG
    run_heads(nh, C, N, N + 1, N + 1, act, True, [0, 64 * C * (nh + 1)])


def test_heads_refuse_nine():
    W, b, X, dY = R.heads_case(8, 5, 1001, 0)
    W9, dY9 = torch.cat([W, W[:1]]), torch.cat([dY, dY[:1]])
    Y, dX, tot, part = full((9, 1001)), full((5, 1001)), full((10, 5)), full((2 * 5 * 10,))
    with pytest.raises(Exception):
        call('tvae_heads_fwd', G(W9), G(X), 1001, None, Y, 1001, 9, 5, 1001)
    with pytest.raises(Exception):
        call('tvae_heads_bwd', G(W9), G(dY9), 1001, G(X), 1001, dX, 1001, 9, 5, 1001, 0, 0.01, part, part.numel(), tot)
    for t in (Y, dX, tot, part):
        assert bool((t == R.SENTINEL).all())


def test_worst_ratios(capsys):
    """Prints the worst ratio of each output over the tests of this file that ran (nothing to assert beyond them)."""
    with capsys.disabled():
        print('\nMLP ends on the GPU: worst error / (u condition) by output, and K')
        for n_, w in WORST.items():
            print(f'  {n_:28s} {w:10.3g}   {R.K.get(n_, "")}')
    assert all(w <= R.K[n_] for n_, w in WORST.items() if n_ in R.K)
