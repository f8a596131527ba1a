"""tests/head_ref.py (the float64 restatement of the attention head) against the fp32 oracle, on the CPU, and the measurement of
the budget constants head_ref.K that test_head_fp64_gpu.py holds the kernels to.  Nothing here runs the code under test."""
import math
import types

import pytest
import torch

import head_ref
from conftest import rel_err

SPACING = 2.0 / 27


def _tables(R, Ho, refine, theta_prior, normal):
    from tvae import tables
    p_r = tables.rotation_log_prior(R, refine, theta_prior, normal)
    tb = types.SimpleNamespace(
        p_r=torch.from_numpy(p_r), off=torch.from_numpy(tables.rotation_offsets(R, refine)),
        grid=torch.from_numpy(tables.translation_grid(Ho, SPACING)).float(),
        p_tr=torch.from_numpy(tables.joint_log_prior(Ho, SPACING, p_r)), sigma_p=math.pi / R,
        theta_off_scale=1.0 if refine else 0.0)
    return head_ref.tables_f64(tb)


# refine on / off and the normal prior over rotations: the first three cases of test_hip_primitives.py::test_attn_head, with its
# inputs, its upstream coefficients and its tolerances
@pytest.mark.parametrize('R,Ho,zd,refine,normal,scale', [(8, 17, 2, True, False, 1.0), (4, 9, 3, False, False, 4.0),
                                                         (16, 5, 2, True, True, 8.0)])
def test_head_ref_agrees_with_the_fp32_oracle(R, Ho, zd, refine, normal, scale):
    from test_hip_primitives import _head_reference, rnd
    B, RP = 3, R * Ho * Ho
    theta_prior = math.pi / 4 if normal else math.pi
    hd = rnd(3 + 2 * zd, B * RP, seed=1, scale=0.5)
    hd[0] *= scale
    E = torch.empty(B, RP).exponential_(generator=torch.Generator().manual_seed(2))
    eps_z, eps_t = rnd(B, zd, seed=3), rnd(B, seed=4)
    hr = hd.clone().requires_grad_(True)
    ref = _head_reference(hr, E, eps_z, eps_t, R, Ho, zd, refine, theta_prior, normal, SPACING)
    coef = [0.3, 0.2, 5.0, 1.0, 1.0, 1.0, 1.0]
    ups = [c * rnd(*r_.shape, seed=20 + i) for i, (c, r_) in enumerate(zip(coef, ref))]
    sum((r_ * u_.to(r_.dtype)).sum() for r_, u_ in zip(ref, ups)).backward()
    outs, _, dh, _ = head_ref.head_with_grad(hd.double().view(-1, B, RP), E, eps_z, eps_t,
                                             _tables(R, Ho, refine, theta_prior, normal), ups)
    for nm, r_, o_ in zip(head_ref.NAMES, ref, outs):
        assert rel_err(r_.detach().reshape(-1), o_.reshape(-1)) < 5e-5, nm
    assert rel_err(hr.grad, dh.reshape(hr.shape)) < 2e-4


# the square-grid shapes of test_head_fp64_gpu.py (register, strided and chunked sizes), z_dim 1 / 2 / 5 / 9 spread over them
BUDGET_CASES = [(4, 5, 1), (8, 17, 2), (8, 33, 5), (16, 24, 9), (4, 64, 2), (8, 66, 5)]


def test_budget_constants(capsys):
    """K of head_ref: fp32 on the CPU (_head_reference and its autograd) against head_ref, on the inputs of the GPU test (plain
    and peaked, refine on and off, seven and four upstream gradients).  K = max(16, 8 x worst ratio); the constants in
    head_ref.K have to cover what is measured here.  The ratios are printed (pytest -s)."""
    from test_hip_primitives import _head_reference
    B = 3
    worst = {n_: 0.0 for n_ in head_ref.K}
    for R, Ho, zd in BUDGET_CASES:
        RP = R * Ho * Ho
        for refine in (False, True):
            tabs = _tables(R, Ho, refine, math.pi, False)
            for peaked in (False, True):
                hd, E, eps_z, eps_t = head_ref.case_inputs(RP, zd, peaked)
                for seven in (True, False):
                    ups = head_ref.upstream(B, RP, zd, seven)
                    hr = hd.clone().requires_grad_(True)
                    f32 = _head_reference(hr, E, eps_z, eps_t, R, Ho, zd, refine, math.pi, False, SPACING)
                    sum((r_ * u_.to(r_.dtype).view_as(r_)).sum() for r_, u_ in zip(f32, ups) if u_ is not None).backward()
                    ref = head_ref.head_with_grad(hd.double().view(-1, B, RP), E, eps_z, eps_t, tabs, ups)
                    r = head_ref.ratios([t.detach() for t in f32], hr.grad, *ref)
                    for n_ in worst:
                        assert math.isfinite(r[n_]), (n_, R, Ho, zd, refine, peaked, seven)
                        worst[n_] = max(worst[n_], r[n_])
    with capsys.disabled():
        print('\nhead budget: worst ratio error / (u condition), fp32 CPU oracle against head_ref, and K = max(16, 8 x ratio)')
        for n_, w in worst.items():
            print(f'  {n_:7s} ratio {w:8.3f}   K measured {max(16.0, 8 * w):8.2f}   K used {head_ref.K[n_]:8.2f}')
    for n_, w in worst.items():
        assert max(16.0, 8 * w) <= head_ref.K[n_], (n_, w, head_ref.K[n_])
        assert head_ref.K[n_] <= max(16.0, 8 * w) * 1.25, (n_, w, head_ref.K[n_], 'K is wider than the measurement allows')


def test_coord_budget_constants(capsys):
    """K of coord_ref: the fp32 torch expression of test_hip_primitives.py::test_coord and its autograd, on the CPU, against
    coord_ref on every case of test_coord_fp64_gpu.py.  Printed; coord_ref.K has to cover it."""
    import coord_ref
    worst = {n_: 0.0 for n_ in coord_ref.K}
    for B, Np in coord_ref.CASES:
        xc, dx, th, g = coord_ref.case(B, Np)
        dx32, th32 = dx.clone().requires_grad_(True), th.clone().requires_grad_(True)
        xr = coord_ref.transform(xc, dx32, th32)
        (xr * g).sum().backward()
        r = coord_ref.ratios((xr, dx32.grad, th32.grad), *coord_ref.reference(xc, dx, th, g))
        for n_ in worst:
            assert math.isfinite(r[n_]), (n_, B, Np)
            worst[n_] = max(worst[n_], r[n_])
    with capsys.disabled():
        print('\ncoordinate budget: worst ratio error / (u condition), fp32 CPU against coord_ref, and K = max(16, 8 x ratio)')
        for n_, w in worst.items():
            print(f'  {n_:7s} ratio {w:8.3f}   K measured {max(16.0, 8 * w):8.2f}   K used {coord_ref.K[n_]:8.2f}')
    for n_, w in worst.items():
        assert max(16.0, 8 * w) <= coord_ref.K[n_] <= max(16.0, 8 * w) * 1.25, (n_, w, coord_ref.K[n_])
