"""Coordinate transform (tvae_coord_fwd / _bwd through tvae.ops.CoordFn) against tests/coord_ref.py in float64: theta up to
+-20 rad, dx up to +-1, Np = 81 / 784 / 33 x 31 / 4096 + 37 (the backward is one 256-thread workgroup per image striding over
Np: one to seventeen trips), B = 1 / 3 / 300 and B = 2675 at Np = 784, where the forward's grid-stride loop takes a second round
(grid1d caps the grid at 8192 workgroups of 256 threads; B = 300 does not get there).

Forward per element, backward per image and component, against K u (condition quantity), u = 2^-24; condition quantities in
coord_ref's docstring.  K: fp32 torch on the CPU against coord_ref on these inputs, 8 x the worst ratio and not below 16
(tests/test_head_ref_cpu.py::test_coord_budget_constants measures and prints them):

    quantity   forward   d dx   d theta
    ratio      2.79      0.39   0.57
    K          23        16     16"""
import math

import pytest
import torch

import coord_ref
import guardband

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in test_hip_primitives.py: every C-ABI call on relocated tensors between guard bands, twice from the same inputs."""
    with guardband.GuardedCalls(replay=True):
        yield


@pytest.mark.parametrize('B,Np', coord_ref.CASES)
def test_coord_fp64(B, Np):
    from tvae import ops
    dev = torch.device('cuda:0')
    xc, dx, th, g = coord_ref.case(B, Np)
    if B == 2675:
        assert B * Np > 8192 * 256 >= (B - 1) * Np            # the smallest B whose forward takes a second grid-stride round
    dxg, thg = dx.to(dev).requires_grad_(True), th.to(dev).requires_grad_(True)
    xr = ops.CoordFn.apply(xc.to(dev), dxg, thg)
    (xr * g.to(dev)).sum().backward()
    torch.cuda.synchronize()
    ref, cond = coord_ref.reference(xc, dx, th, g)
    r = coord_ref.ratios((xr, dxg.grad, thg.grad), ref, cond)
    print((B, Np), {k_: round(v, 3) for k_, v in r.items()})
    for n_, k_ in coord_ref.K.items():
        assert math.isfinite(r[n_]) and r[n_] <= k_, (n_, r[n_], k_)
