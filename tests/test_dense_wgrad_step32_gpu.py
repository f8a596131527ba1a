"""The sign-bit weight gradient of the decoder (tvae_linear_wgrad_x6 from stored sign bits against gy x the recomputed
first-layer activation) at the shapes that decide between its 32-column and its 16-column instance, against float64 on the
host.  The bit WORDS are drawn directly as random int32 (no forward pass): no element sits at zero to rounding, so the
comparison is free of mask flips and every arithmetic is held to its plain bound.

With M = K = 512 the reduction is cut into 128 slices, so N = 128 * nchunk and a slice is nchunk / 32 steps of the 32-column
instance: 1, 2, 3, 4, 5, 8 and 9 steps cover the clamped prologue (fewer steps than the ring is deep), odd and even trip counts
of the loop unrolled by two, and more steps than ring slots.  Np puts image boundaries (where the latent term changes) at step
boundaries inside a slice, at slice boundaries and once per tensor.  Np = 48 is not a multiple of 32 and must take the
16-column instance; it is checked like the others."""
import pytest
import torch

import guardband
from conftest import rel_err
from dense_bits_ref import random_bits

pytestmark = pytest.mark.gpu
SLOPE = 0.01
GEMM_TOL = {'f32': 2e-5}          # tests/test_hip_primitives.py
BF16_TOL = 1.5e-2                 # one-part mode: the bound of test_conv1_dft_bf16_mode


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in tests/test_hip_primitives.py: every call runs on relocated tensors between guard bands, twice."""
    with guardband.GuardedCalls(replay=True):
        yield


def dev():
    return torch.device('cuda:0')


def call(*a, **kw):
    from tvae._lib import call as c
    return c(*a, **kw)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def first_layer_fp64(xr, Wc, bc, LB, Np):
    """H0[k][n] = LeakyReLU(Wc[k] . x'[n] + bc[k] + LB[n // Np][k]) in float64."""
    img = torch.arange(xr.shape[0]) // Np
    pre = xr.double() @ Wc.double().t() + bc.double()[None, :] + LB.double()[img]
    return torch.where(pre > 0, pre, SLOPE * pre).t().contiguous()


# (M, K, N, Np): nchunk = N / 128 at M = K = 512 (128 slices); see the module docstring
SHAPES = [
    (512, 512, 128 * 32, 32),           # 1 step per slice, an image per slice
    (512, 512, 128 * 64, 64),           # 2 steps, image boundaries at slice boundaries
    (512, 512, 128 * 96, 96),           # 3 steps (= ring depth)
    (512, 512, 128 * 128, 64 * 128),    # 4 steps, one image boundary in the tensor (Np = N / 2)
    (512, 512, 128 * 160, 32),          # 5 steps, an image boundary at every step
    (512, 512, 128 * 256, 64),          # 8 steps, a boundary every second step
    (512, 512, 128 * 288, 96),          # 9 steps, a boundary every third step
    (512, 512, 12224, 32),              # nchunk 96; the last slice is a single step (12 224 - 127 * 96 = 32)
    (200, 200, 256 * 64, 32),           # clamped rows and a partial k tile: 2 k tiles -> 256 slices of 64 columns
    (512, 512, 128 * 96, 48),           # Np % 32 != 0: the 16-column instance
]


@pytest.mark.parametrize('M,K,N,Np', SHAPES)
def test_wgrad_from_bits_against_fp64(M, K, N, Np):
    from tvae._lib import query
    assert N % Np == 0
    B = N // Np
    xr, Wc, bc, LB = rnd(N, 2, seed=1), rnd(K, 2, seed=2), rnd(K, seed=3), rnd(B, K, seed=4)
    W, wo, gy = rnd(M, K, seed=5, scale=K ** -0.5), rnd(M, seed=8), rnd(N, seed=9)
    words, mask = random_bits(M, N, seed=10)
    H0 = first_layer_fp64(xr, Wc, bc, LB, Np)
    dact = torch.where(mask, 1.0, SLOPE).double()
    G = (gy.double()[None, :] * dact) @ H0.t()                     # dW before the row factor wo[m]
    ref_dW = wo.double()[:, None] * G
    ref_rd = (W.double() * G).sum(1)
    dv = [t.to(dev()) for t in (xr, Wc, bc, LB, W, wo, gy, words)]
    xr_d, Wc_d, bc_d, LB_d, W_d, wo_d, gy_d, bits_d = dv
    ws = torch.empty(query('tvae_linear_wgrad_x6_ws_floats', M, N, K), device=dev())
    for parts in (3, 2, 1):
        tol = GEMM_TOL['f32'] if parts > 1 else BF16_TOL
        dW = torch.full((M, K), float('nan'), device=dev())
        rd = torch.full((M,), float('nan'), device=dev())
        call('tvae_linear_wgrad_x6', None, None, dW, ws, ws.numel(), M, N, K, N, N, 0, vg_wo=wo_d, vg_gy=gy_d, vg_act=1,
             vg_slope=SLOPE, va_xr=xr_d, va_wc=Wc_d, va_bc=bc_d, va_lb=LB_d, va_np=Np, vg_bits=bits_d, parts=parts, rd_w=W_d,
             rd_ldw=K, rd_rowdot=rd)
        e_dw, e_rd = rel_err(dW, ref_dW), rel_err(rd, ref_rd)
        print('M %d K %d N %d Np %d parts %d: rel_err dW %.3g rowdot %.3g' % (M, K, N, Np, parts, e_dw, e_rd))
        assert torch.isfinite(dW).all() and torch.isfinite(rd).all()
        assert e_dw < tol, (parts, e_dw)
        assert e_rd < tol, (parts, e_rd)
