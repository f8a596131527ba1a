"""tests/mlp_ends_ref.py checked on the CPU: its gradient restatements against torch autograd in float64 (with the activation
derivative taken from the stored output, the planted +-0.0 / +-1e-30 / 1 - 2^-24 included), its case lists against the branch
conditions they are meant to reach, and its K table against fp32 torch on the CPU on the very cases
test_mlp_ends_fp64_gpu.py runs (K = max(16, 8 x worst ratio); printed by test_budget_constants)."""
import math

import pytest
import torch

import mlp_ends_ref as R

F64 = torch.float64


def pre_of(H, act):
    """A float64 pre-activation whose activation is the stored output H, with leaky ReLU's kink exactly where H is +-0.0."""
    H = H.double()
    if act == 1:
        return torch.where(H > 0, H, H / R.SLOPE)
    return torch.atanh(H) if act == 2 else H


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('act', [0, 1, 2])
def test_activation_derivative_convention(act):
    y = torch.tensor(R.SPECIALS + [0.5, -0.5, 1.0, -1.0], dtype=torch.float32)
    d = R.dact(y, act)
    if act == 1:
        assert d.tolist() == [R.SLOPE, R.SLOPE, 1.0, R.SLOPE, 1.0, R.SLOPE, 1.0, R.SLOPE, 1.0, R.SLOPE]      # slope at +0.0 AND -0.0
    elif act == 2:
        assert d[4] == 1 - R.ONE_M ** 2 and d[4] > 0 and d[8] == 0 and d[0] == 1
        assert float(R.dact(y, act, cond=True)[4]) == 1 + R.ONE_M ** 2
    else:
        assert (d == 1).all()
    # autograd of the activation itself at a pre-activation that gives y
    if act:
        p = pre_of(y[:8], act).requires_grad_(True)
        R.act_apply(p, act).sum().backward()
        assert close(p.grad, R.dact(y[:8], act), 1e-7)


@pytest.mark.parametrize('no,act', [(1, 1), (3, 2), (4, 0)])
def test_last_layer_gradients_against_autograd(no, act):
    """outer_mask and dec_out_bwd are d/d pre of y = Wo act(pre) + bo; coldot is that y; act_bwd the mask alone."""
    H, W, b, dy = R.skinny_case(no, act)
    pre = pre_of(H, act).requires_grad_(True)
    W64 = W.double().requires_grad_(True)
    y = (W64 @ R.act_apply(pre, act)).t() + b.double()
    assert close(R.coldot(R.act_apply(pre, act).detach(), W, b), y.detach())
    (y * dy.double()).sum().backward()
    D = R.outer_mask(dy, W, H, act)
    assert close(D, pre.grad, 1e-7)
    out = R.dec_out_bwd(dy, W, H, act)
    assert close(out['out_D'], pre.grad, 1e-7) and close(out['out_tot'][0], pre.grad.sum(1), 1e-7)
    assert close(out['out_tot'][1:], W64.grad, 1e-7)          # (H is act(pre) to a rounding of atanh)
    dY, p = R.rnd(*H.shape, seed=5), pre_of(H, act).requires_grad_(True)
    (R.act_apply(p, act) * dY.double()).sum().backward()
    assert close(R.act_bwd(dY, H, act), p.grad, 1e-7)


@pytest.mark.parametrize('nh,C,act', [(1, 5, 1), (7, 33, 2), (8, 5, 0)])
def test_head_projection_gradients_against_autograd(nh, C, act):
    """heads_fwd is Y = W X + b with X = act(pre + bx); heads_bwd gives d/d pre, dW and d/d bx (the bias of the layer before)."""
    W, b, X, dY = R.heads_case(nh, C, 1001, act)
    pre = pre_of(X, act).requires_grad_(True)
    w, bx = W.double().requires_grad_(True), torch.zeros(C, 1, dtype=F64, requires_grad=True)
    Y = w @ R.act_apply(pre + bx, act) + b.double()[:, None]
    assert close(R.heads_fwd(W, R.act_apply(pre, act).detach(), b), Y.detach())
    (Y * dY.double()).sum().backward()
    got = R.heads_bwd(W, dY, X, act)
    assert close(got['heads_dX'], pre.grad, 1e-7)
    assert close(got['heads_tot'][:nh], w.grad, 1e-7) and close(got['heads_tot'][nh], bx.grad[:, 0], 1e-7)


@pytest.mark.parametrize('F,B,Np,ldd', R.DEC_IN_CASES[:3])
def test_first_layer_gradients_against_autograd(F, B, Np, ldd):
    d, xr, Wc = R.dec_in_case(F, B, Np)
    x, w = xr.double().requires_grad_(True), Wc.double().requires_grad_(True)
    bc, lb = torch.zeros(F, dtype=F64, requires_grad=True), torch.zeros(B, F, dtype=F64, requires_grad=True)
    pre = x @ w.t() + bc + lb.repeat_interleave(Np, 0)
    (pre.t() * d.double()).sum().backward()
    got = R.dec_in_bwd(d, xr, Wc, B, Np)
    for n_, g in (('in_gxr', x.grad), ('in_Simg', lb.grad), ('in_dbc', bc.grad), ('in_dWc', w.grad)):
        assert close(got[n_], g), n_


@pytest.mark.parametrize('F,zd,act,has_lb', R.L0_CASES)
def test_first_layer_forward_and_latent(F, zd, act, has_lb):
    xr, Wc, bc, Wl, z = R.l0_case(F, zd)
    z64, wl = z.double().requires_grad_(True), Wl.double().requires_grad_(True)
    LB = z64 @ wl.t()
    assert close(R.latent_bias(Wl, z), LB.detach())
    S = R.rnd(R.L0_B, F, seed=1)
    (LB * S.double()).sum().backward()
    g = R.latent_bwd(S, Wl, z)
    assert close(g['dWl'], wl.grad) and close(g['dz'], z64.grad)
    lb32 = LB.detach().float() if has_lb else None
    h = R.dec_l0_fwd(xr, Wc, bc, lb32, R.L0_NP, act)
    want = torch.stack([R.act_apply(xr[n].double() @ Wc.double().t() + bc.double() +
                                    (lb32[n // R.L0_NP].double() if has_lb else 0), act) for n in (0, 99, 100, 299)], 1)
    assert close(h[:, [0, 99, 100, 299]], want)
    c = R.dec_l0_fwd(xr, Wc, bc, lb32, R.L0_NP, act, cond=True)
    assert c.shape == h.shape and (c >= h.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize('F,sigma', [(5, 2.0 / 27), (257, 0.01)])
def test_fourier_gradient_against_autograd(F, sigma):
    """In float64 throughout (x64 w64 + b): the restatement differs from it by the rounding of the fp32 argument only, which its
    condition quantity covers."""
    xr, Wf, bf, g = R.fourier_case(F)
    w = R.fourier_arg(xr, Wf, bf, sigma)[0]
    x = xr.double().requires_grad_(True)
    feat = torch.cos(x @ w.double().t() + bf.double()).t()
    (feat * g.double()).sum().backward()
    for ref, cond, want in ((*R.both(R.fourier_fwd, xr, Wf, bf, sigma), feat.detach()),
                            (*R.both(R.fourier_bwd, xr, Wf, bf, sigma, g), x.grad)):
        assert float(((ref - want).abs() / (R.U * cond)).max()) < 4.0


def test_case_lists_reach_their_branches():
    """The arithmetic of the branch conditions (csrc/small_kernels.hpp, fused_tail_kernels.hpp, abi_small.hip) on the case lists."""
    forms = {}
    for seglen, N in R.ROWSUM_SHAPES:
        for nbeg in range(0, N, seglen):
            n4 = (min(N, nbeg + seglen) - nbeg) // 4
            forms.setdefault(seglen, set()).add(('dword' if nbeg % 4 else '16-byte', n4 > 256, n4 > 768, n4 % 256 != 0,
                                                 (min(N, nbeg + seglen) - nbeg) % 4))
    assert all(not f[1] for f in forms[300]) and any(f[0] == '16-byte' and f[1] and not f[2] for f in forms[1600])
    assert any(f[0] == '16-byte' and f[2] and f[4] == 3 for f in forms[3151]) and any(f[0] == 'dword' for f in forms[3151])
    assert any(N < seglen for seglen, N in R.ROWSUM_SHAPES) and all(N % seglen for seglen, N in R.ROWSUM_SHAPES)
    assert all(R.ld_pad4(N) % 4 == 0 and R.ld_pad4(N) >= N + 4 for _, N in R.ROWSUM_SHAPES)
    kern = {(S, L): 'wave' if L <= 64 and S >= 32 else ('tile' if S >= 64 and L <= 65536 else 'plain') for S, L in R.SEG_SUM_CASES}
    assert [kern[c] for c in R.SEG_SUM_CASES] == ['wave', 'plain', 'tile', 'plain', 'tile', 'plain', 'tile', 'tile']
    assert {c[2] for c in R.SKINNY_CASES} == {0, 1, 2} and {c[3] for c in R.SKINNY_CASES} == {True, False}
    vec = [ldh % 4 == 0 and ldd % 4 == 0 for _, _, ldh, ldd, _, _ in R.DEC_OUT_CASES]
    assert vec == [True, False, True, True] and R.DEC_OUT_CASES[2][1] % 4 == 3 and R.DEC_OUT_CASES[0][0] // 16 == 8
    assert {c[4] for c in R.DEC_OUT_CASES} == {1, 2, 3, 4} and {c[5] for c in R.DEC_OUT_CASES} == {0, 1, 2}
    assert [ldd % 4 == 0 and Np % 4 == 0 for _, _, Np, ldd in R.DEC_IN_CASES] == [True, False, True, True]
    assert {c[0] for c in R.HEADS_CASES} == set(range(1, 9)) and {c[3] for c in R.HEADS_CASES} == {0, 1, 2}
    assert {c[4] for c in R.HEADS_CASES} == {True, False} and {c[1] for c in R.HEADS_CASES} == {5, 33}
    for nh in range(1, 9):
        assert {c[2] for c in R.HEADS_CASES if c[0] == nh} == set(R.HEADS_LAYOUTS)
    nh, C, N, _ = R.HEADS_BIG
    assert (N + 511) // 512 >= 4 * 64 and (C * (nh + 1)) % 4 == 0


def f32_ratios():
    """name -> worst ratio of the fp32 CPU evaluation against the reference, over every case of the GPU file."""
    worst = {n_: 0.0 for n_ in R.K}

    def take(name, fn, *args, floor=None):
        ref, cond = R.both(fn, *args)
        got = fn(*args, dt=torch.float32)
        if not isinstance(ref, dict):
            ref, cond, got = {name: ref}, {name: cond}, {name: got}
        for n_, r in R.ratios(got, ref, cond, floor).items():
            assert math.isfinite(r), (n_, args[-1])
            worst[n_] = max(worst[n_], r)

    for seglen, N in R.ROWSUM_SHAPES:
        take('rowdot', R.rowdot_seg, R.rowsum_case(seglen, N), None, seglen)
    for no in R.ROWDOT_V_CASES:
        take('rowdot', R.rowdot_seg, *R.rowdot_v_case(no), 500)
    for (S, L), (scale, acc) in ((c, m) for c in R.SEG_SUM_CASES for m in R.SEG_SUM_MODES):
        take('seg_sum', R.seg_sum, *R.seg_sum_case(S, L), scale, acc)
    for no, lay, act, has_b in R.SKINNY_CASES:
        H, W, b, dy = R.skinny_case(no, act)
        take('coldot', R.coldot, H, W, b if has_b else None)
        take('outer_mask', R.outer_mask, dy, W, H, act)
        take('act_bwd', R.act_bwd, R.rnd(*H.shape, seed=5), H, act)
    for F, zd, act, has_lb in R.L0_CASES:
        xr, Wc, bc, Wl, z = R.l0_case(F, zd)
        take('latent_bias', R.latent_bias, Wl, z)
        take('dec_l0', R.dec_l0_fwd, xr, Wc, bc, R.latent_bias(Wl, z).float() if has_lb else None, R.L0_NP, act)
    for c in R.LATENT_BWD_CASES:
        take(None, R.latent_bwd, *R.latent_bwd_case(*c))
    for F, sigma in R.FOURIER_FWD_CASES:
        take('fourier_fwd', R.fourier_fwd, *R.fourier_case(F)[:3], sigma)
    for F, sigma in R.FOURIER_BWD_CASES:
        xr, Wf, bf, g = R.fourier_case(F)
        take('fourier_bwd', R.fourier_bwd, xr, Wf, bf, sigma, g)         # (no floor: the CPU's sine needs none)
    for F, N, ldh, ldd, no, act in R.DEC_OUT_CASES:
        take(None, R.dec_out_bwd, *R.dec_out_case(F, N, no, act), act)
    for F, B, Np, ldd in R.DEC_IN_CASES:
        take(None, R.dec_in_bwd, *R.dec_in_case(F, B, Np), B, Np)
    for nh, C, N, act in [(nh, C, lay[0], act) for nh, C, lay, act, _ in R.HEADS_CASES] + [R.HEADS_BIG]:
        W, b, X, dY = R.heads_case(nh, C, N, act)
        take('heads_Y', R.heads_fwd, W, X, b)
        take(None, R.heads_bwd, W, dY, X, act)
    return worst


def test_budget_constants(capsys):
    """K of mlp_ends_ref: every operation in fp32 torch on the CPU against its float64 restatement, on every case of
    test_mlp_ends_fp64_gpu.py.  Printed; mlp_ends_ref.K has to cover it, and not by more than a quarter."""
    worst = f32_ratios()
    with capsys.disabled():
        print('\nMLP-end budgets: worst ratio error / (u condition), fp32 CPU against mlp_ends_ref, and K = max(16, 8 x ratio)')
        for n_, w in worst.items():
            print(f'  {n_:12s} ratio {w:8.3f}   K measured {max(16.0, 8 * w):8.2f}   K used {R.K[n_]:8.2f}')
    for n_, w in worst.items():
        assert w > 0, n_                                     # (every output was measured)
        assert max(16.0, 8 * w) <= R.K[n_] <= max(16.0, 8 * w) * 1.25, (n_, w, R.K[n_])


def test_ratio_helper_is_strict():
    ref, cond = torch.tensor([1.0, 2.0, 0.0], dtype=F64), torch.tensor([1.0, 2.0, 0.0], dtype=F64)
    assert R.ratio(ref.float(), ref, cond) == 0.0
    assert R.ratio(torch.tensor([1.0, 2.0, 1e-30]), ref, cond) == math.inf            # exact where the condition is zero
    assert R.ratio(torch.tensor([1.0, float('nan'), 0.0]), ref, cond) == math.inf
    assert abs(R.ratio(torch.tensor([1.0 + 2.0 ** -20, 2.0, 0.0]), ref, cond) - 16.0) < 1e-6
    assert R.ratio(torch.tensor([1.0 + 2.0 ** -20, 2.0, 0.0]), ref, cond, floor=torch.full((3,), 1.0, dtype=F64)) == 0.0
