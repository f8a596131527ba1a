"""GPU parity of every C-ABI entry point of libtvae_hip.so against plain torch fp64/fp32 math.
These call through the C ABI (tvae._lib.call -> ctypes) on cuda:0."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guardband
from conftest import rel_err
from oracle import tvae_oracle as O

pytestmark = pytest.mark.gpu
TOL = 2e-5
SLOPE = 0.01
# per-tensor relative tolerance of the fp32-MFMA entry points (the *_x6 / *_dft entry points are held to the same
# number in their own tests below); the hot-path parity gate is 1e-4 (BASELINE.json north_star)
GEMM_TOL = {'f32': 2e-5}


@pytest.fixture(params=['f32'])
def gemm_mode(request):
    return request.param


@pytest.fixture(autouse=True)
def guarded_calls():
    """Every test of this file runs each of its C-ABI calls on relocated tensors between guard bands, twice from the same
    inputs (tests/guardband.py): a store outside a tensor, a read outside one that reaches a result, and a result that
    differs between two runs all fail the test (reported at teardown, with the call).  No test runs with replay off."""
    with guardband.GuardedCalls(replay=True):
        yield


def dev():
    return torch.device('cuda:0')


def call(*a, **kw):
    from tvae._lib import call as c
    return c(*a, **kw)


def query(*a):
    from tvae._lib import query as q
    return q(*a)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale)


def act_ref(x, act):
    return x if act == 0 else (F.leaky_relu(x, SLOPE) if act == 1 else torch.tanh(x))


def dact_ref(y, act):
    if act == 0:
        return torch.ones_like(y)
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE)) if act == 1 else 1 - y * y


@pytest.mark.parametrize('M,N,K,act,use_g,use_res', [
    (128, 8712, 128, 1, False, False), (7, 300, 128, 0, False, False), (512, 1000, 1024, 1, True, False),
    (64, 517, 64, 1, False, True), (130, 129, 17, 2, True, True), (103, 2000, 128, 0, False, False),
    (128, 1024, 128, 1, True, True), (256, 512, 64, 0, False, False), (512, 2048, 512, 1, True, False),
    (128, 1024, 128, 1, False, True), (256, 1152, 32, 2, False, True), (384, 128, 16, 1, False, False)])
def test_linear_fwd(M, N, K, act, use_g, use_res, gemm_mode):
    W, X, b = rnd(M, K, seed=1, scale=K ** -0.5), rnd(K, N, seed=2), rnd(M, seed=3)
    group = 100
    ng = (N + group - 1) // group
    gb = rnd(ng, M, seed=4) if use_g else None
    res = rnd(M, N, seed=5) if use_res else None
    ref = W.double() @ X.double() + b.double()[:, None]
    if use_g:
        ref = ref + gb.double()[torch.arange(N) // group].t()
    if use_res:
        ref = ref + res.double()
    ref = act_ref(ref, act)
    Y = torch.empty(M, N, device=dev())
    call('tvae_linear_fwd', W.to(dev()), X.to(dev()), b.to(dev()), gb.to(dev()) if use_g else None, group,
         res.to(dev()) if use_res else None, Y, M, N, K, N, N, act, SLOPE)
    assert rel_err(Y, ref) < GEMM_TOL[gemm_mode]


@pytest.mark.parametrize('M,N,K,mask,use_add', [(7, 3000, 128, 1, False), (128, 1111, 128, 1, False),
                                                (64, 300, 64, 1, True), (512, 700, 1024, 0, False),
                                                (33, 257, 65, 2, True), (128, 1024, 128, 1, True), (64, 512, 256, 1, False),
                                                (512, 1024, 512, 0, False), (128, 512, 256, 2, True), (16, 1280, 384, 1, False)])
def test_linear_dgrad(M, N, K, mask, use_add, gemm_mode):
    W, d = rnd(M, K, seed=1, scale=M ** -0.5), rnd(M, N, seed=2)
    aux = rnd(K, N, seed=3).clamp(-0.9, 0.9)
    add = rnd(K, N, seed=4) if use_add else None
    ref = W.double().t() @ d.double()
    if use_add:
        ref = ref + add.double()
    ref = ref * dact_ref(aux.double(), mask)
    dX = torch.empty(K, N, device=dev())
    call('tvae_linear_dgrad', W.to(dev()), d.to(dev()), add.to(dev()) if use_add else None,
         aux.to(dev()) if mask else None, dX, M, N, K, N, N, mask, SLOPE)
    assert rel_err(dX, ref) < GEMM_TOL[gemm_mode]


@pytest.mark.parametrize('M,N,K,acc', [(7, 50000, 128, 0), (128, 8712 * 3, 128, 0), (64, 1000, 2, 1),
                                       (512, 20000, 512, 0), (130, 777, 1024, 0), (128, 8192, 128, 0), (256, 4096, 512, 1)])
def test_linear_wgrad(M, N, K, acc, gemm_mode):
    d, X = rnd(M, N, seed=1), rnd(K, N, seed=2)
    init = rnd(M, K, seed=3)
    ref = d.double() @ X.double().t() + (init.double() if acc else 0)
    dW = init.clone().to(dev()) if acc else torch.empty(M, K, device=dev())
    ws = torch.empty(1 << 24, device=dev())
    call('tvae_linear_wgrad', d.to(dev()), X.to(dev()), dW, ws, ws.numel(), M, N, K, N, N, acc)
    assert rel_err(dW, ref) < GEMM_TOL[gemm_mode]


def test_linear_wgrad_no_workspace():
    M, N, K = 20, 5000, 30
    d, X = rnd(M, N, seed=1), rnd(K, N, seed=2)
    dW = torch.empty(M, K, device=dev())
    call('tvae_linear_wgrad', d.to(dev()), X.to(dev()), dW, None, 0, M, N, K, N, N, 0)
    assert rel_err(dW, d.double() @ X.double().t()) < TOL


@pytest.mark.parametrize('k,R,Cin,C', [(5, 4, 1, 3), (28, 8, 1, 4), (9, 16, 3, 2), (7, 8, 3, 11), (32, 8, 1, 128)])
def test_rotate_bank(k, R, Cin, C):
    from tvae import ops
    w = rnd(C, Cin, 1, k, k, seed=k)
    wr = w.clone().requires_grad_(True)
    ref = O.rotated_bank(wr, R)                      # (C,R,Cin,1,k,k)
    wg = w.to(dev()).requires_grad_(True)
    bank = ops.BankFn.apply(wg, R)
    assert rel_err(bank.view(C, R, Cin, 1, k, k), ref) < 1e-6
    g = rnd(*ref.shape, seed=9)
    (ref * g).sum().backward()
    (bank.view(C, R, Cin, 1, k, k) * g.to(dev())).sum().backward()
    assert rel_err(wg.grad, wr.grad) < 1e-5


@pytest.mark.parametrize('B,Cin,n,k,pad,C,R,act', [(2, 1, 28, 28, 8, 8, 8, 1), (3, 3, 12, 9, 3, 4, 4, 0),
                                                   (2, 1, 64, 64, 16, 4, 8, 1), (5, 2, 20, 7, 0, 3, 16, 0),
                                                   (3, 1, 64, 64, 16, 16, 8, 1), (2, 2, 40, 32, 6, 32, 4, 0),
                                                   (2, 1, 20, 16, 3, 8, 16, 1)])
def test_conv1_fwd_wgrad(B, Cin, n, k, pad, C, R, act, gemm_mode):
    y = torch.rand(B, Cin, n, n, generator=torch.Generator().manual_seed(1))
    bank = rnd(C * R, Cin * k * k, seed=2, scale=(Cin * k * k) ** -0.5)
    bias = rnd(C, seed=3, scale=0.1)
    Ho = n + 2 * pad - k + 1
    ref = F.conv2d(y.double(), bank.double().view(C * R, Cin, k, k), None, 1, pad).view(B, C, R, Ho, Ho) \
        + bias.double().view(1, C, 1, 1, 1)
    ref = act_ref(ref, act)
    out = torch.empty(C, B * R * Ho * Ho, device=dev())
    call('tvae_conv1_fwd', y.to(dev()), bank.to(dev()), bias.to(dev()), out, B, Cin, n, k, pad, C, R, act, SLOPE)
    got = out.view(C, B, R, Ho, Ho).permute(1, 0, 2, 3, 4)
    assert rel_err(got, ref) < GEMM_TOL[gemm_mode]
    # weight gradient
    g = rnd(B, C, R, Ho, Ho, seed=4)
    ref_g = torch.nn.grad.conv2d_weight(y.double(), (C * R, Cin, k, k), g.double().view(B, C * R, Ho, Ho), padding=pad)
    dpre = g.permute(1, 0, 2, 3, 4).contiguous().view(C, -1).to(dev())
    dbank = torch.empty(C * R, Cin * k * k, device=dev())
    ws = torch.empty(1 << 22, device=dev())
    call('tvae_conv1_wgrad', y.to(dev()), dpre, dbank, ws, ws.numel(), B, Cin, n, k, pad, C, R)
    assert rel_err(dbank.view(C * R, Cin, k, k), ref_g) < GEMM_TOL[gemm_mode]


@pytest.mark.parametrize('B,Cin,n,k,pad,C,R,act', [(2, 1, 28, 28, 8, 8, 8, 1), (3, 3, 12, 9, 3, 4, 4, 0),
                                                   (2, 1, 64, 64, 16, 4, 8, 1), (5, 2, 20, 7, 0, 3, 16, 0),
                                                   (3, 1, 64, 64, 16, 16, 8, 1), (2, 1, 40, 32, 6, 32, 4, 0),
                                                   (2, 1, 20, 16, 3, 8, 16, 1), (17, 1, 64, 64, 16, 48, 8, 1)])
def test_conv1_x6_matches_fp64_at_fp32_tolerance(B, Cin, n, k, pad, C, R, act):
    """3xbf16-split conv kernels: same tolerance as the exact-fp32 MFMA path (GEMM_TOL['f32'])."""
    from tvae._lib import query
    if not query('tvae_conv1_x6_supported', Cin, n, k, pad):
        pytest.skip('geometry does not fit the LDS-resident x6 kernels')
    y = torch.rand(B, Cin, n, n, generator=torch.Generator().manual_seed(1))
    bank = rnd(C * R, Cin * k * k, seed=2, scale=(Cin * k * k) ** -0.5)
    bias = rnd(C, seed=3, scale=0.1)
    Ho = n + 2 * pad - k + 1
    ref = F.conv2d(y.double(), bank.double().view(C * R, Cin, k, k), None, 1, pad).view(B, C, R, Ho, Ho) \
        + bias.double().view(1, C, 1, 1, 1)
    ref = act_ref(ref, act)
    a3 = torch.empty(query('tvae_conv1_x6_bank_bytes', C, R, Cin, k) // 4, device=dev())
    call('tvae_bank_split3', bank.to(dev()), a3, a3.numel() * 4, C, R, Cin, k)
    out = torch.empty(C, B * R * Ho * Ho, device=dev())
    call('tvae_conv1_fwd_x6', y.to(dev()), a3, bias.to(dev()), out, B, Cin, n, k, pad, C, R, act, SLOPE)
    got = out.view(C, B, R, Ho, Ho).permute(1, 0, 2, 3, 4)
    assert rel_err(got, ref) < GEMM_TOL['f32']
    g = rnd(B, C, R, Ho, Ho, seed=4)
    ref_g = torch.nn.grad.conv2d_weight(y.double(), (C * R, Cin, k, k), g.double().view(B, C * R, Ho, Ho), padding=pad)
    dpre = g.permute(1, 0, 2, 3, 4).contiguous().view(C, -1).to(dev())
    dbank = torch.empty(C * R, Cin * k * k, device=dev())
    ws = torch.empty(1 << 22, device=dev())
    d3 = torch.empty(query('tvae_conv1_x6_dy_bytes', B, C, R, n, k, pad) // 4, device=dev())
    call('tvae_dy_split3', dpre, d3, d3.numel() * 4, B, Cin, n, k, pad, C, R)
    call('tvae_conv1_wgrad_x6', y.to(dev()), d3, dbank, ws, ws.numel(), B, Cin, n, k, pad, C, R)
    assert rel_err(dbank.view(C * R, Cin, k, k), ref_g) < GEMM_TOL['f32']


@pytest.mark.parametrize('M,N,K,act,use_res', [(512, 2048, 512, 1, False), (128, 1024, 128, 1, True), (300, 384, 40, 2, False),
                                               (512, 128, 512, 0, True), (64, 256, 1024, 1, False)])
def test_linear_fwd_dgrad_x6(M, N, K, act, use_res):
    """Dense layers in the exact-split bf16 arithmetic: same tolerance as the fp32 MFMA path."""
    from tvae._lib import query
    W, X, b = rnd(M, K, seed=1, scale=K ** -0.5), rnd(K, N, seed=2), rnd(M, seed=3)
    res = rnd(M, N, seed=5) if use_res else None
    ref = W.double() @ X.double() + b.double()[:, None]
    if use_res:
        ref = ref + res.double()
    ref = act_ref(ref, act)
    w3 = torch.empty(query('tvae_dense_x6_bytes', M, K) // 4, device=dev())
    Wd = W.to(dev())
    call('tvae_dense_split3', Wd, K, w3, w3.numel() * 4, M, K, 0, None, None)
    Y = torch.empty(M, N, device=dev())
    cw, cb = rnd(M, seed=11), rnd(1, seed=12)
    cy = torch.empty(N, device=dev())
    fuse = M <= 512
    call('tvae_linear_fwd_x6', w3, X.to(dev()), b.to(dev()), res.to(dev()) if use_res else None, Y, M, N, K, N, N, act, SLOPE,
         col_w=cw.to(dev()) if fuse else None, col_b=cb.to(dev()) if fuse else None, col_y=cy if fuse else None, parts=3)
    if fuse:
        assert rel_err(cy, cw.double() @ ref + cb.double()) < GEMM_TOL['f32']
    assert rel_err(Y, ref) < GEMM_TOL['f32']
    # data gradient: dX[k][n] = act'(aux) * (add + sum_m W[m][k] d[m][n])
    d = rnd(M, N, seed=6)
    aux = rnd(K, N, seed=7).clamp(-0.9, 0.9)
    add = rnd(K, N, seed=8) if use_res else None
    refg = W.double().t() @ d.double()
    if use_res:
        refg = refg + add.double()
    refg = refg * dact_ref(aux.double(), act)
    w3t = torch.empty(query('tvae_dense_x6_bytes', K, M) // 4, device=dev())
    call('tvae_dense_split3', Wd, K, w3t, w3t.numel() * 4, K, M, 1, None, None)
    dX = torch.empty(K, N, device=dev())
    call('tvae_linear_dgrad_x6', w3t, d.to(dev()), add.to(dev()) if use_res else None, aux.to(dev()) if act else None, dX, M, N,
         K, N, N, act, SLOPE, parts=3)
    assert rel_err(dX, refg) < GEMM_TOL['f32']
    with pytest.raises(Exception):
        call('tvae_linear_fwd_x6', w3, X.to(dev()), b.to(dev()), None, Y, M, N - 1, K, N, N, act, SLOPE, parts=3)


@pytest.mark.parametrize('M,N,K,acc', [(512, 20000 // 16 * 16, 512, 0), (128, 8192, 128, 0), (300, 1600, 70, 1), (512, 4096, 512, 1)])
def test_linear_wgrad_x6(M, N, K, acc):
    d, X = rnd(M, N, seed=1), rnd(K, N, seed=2)
    init = rnd(M, K, seed=3)
    ref = d.double() @ X.double().t() + (init.double() if acc else 0)
    dW = init.clone().to(dev()) if acc else torch.empty(M, K, device=dev())
    ws = torch.empty(1 << 26, device=dev())       # >= tvae_linear_wgrad_x6_ws_floats(M, N, K): slices x M x K
    from tvae._lib import query
    need = query('tvae_linear_wgrad_x6_ws_floats', M, N, K)
    assert 2 * M * K <= need <= ws.numel()
    call('tvae_linear_wgrad_x6', d.to(dev()), X.to(dev()), dW, ws, ws.numel(), M, N, K, N, N, acc, vg_slope=SLOPE, parts=3)
    assert rel_err(dW, ref) < GEMM_TOL['f32']
    dW2 = init.clone().to(dev()) if acc else torch.empty(M, K, device=dev())
    call('tvae_linear_wgrad_x6', d.to(dev()), X.to(dev()), dW2, ws, need, M, N, K, N, N, acc, vg_slope=SLOPE, parts=3)
    assert torch.equal(dW, dW2)          # the summation order does not depend on how much workspace is offered
    with pytest.raises(Exception):
        call('tvae_linear_wgrad_x6', d.to(dev()), X.to(dev()), dW2, ws, need - 1, M, N, K, N, N, acc, vg_slope=SLOPE, parts=3)
    with pytest.raises(Exception):
        call('tvae_linear_wgrad_x6', d.to(dev()), X.to(dev()), dW, ws, ws.numel(), M, N - 8, K, N, N, acc, vg_slope=SLOPE,
             parts=3)


@pytest.mark.parametrize('B,n,k,pad,C,R,act,Cin', [
    (2, 28, 28, 8, 32, 8, 1, 1), (3, 64, 64, 16, 32, 8, 1, 1), (5, 40, 32, 6, 64, 4, 0, 1), (17, 64, 64, 16, 64, 8, 1, 1),
    (4, 32, 32, 8, 16, 8, 1, 1), (3, 20, 9, 2, 5, 4, 0, 1),
    # the three frames of the ring (LDS-DMA) transforms along w, with several tiles per wave (steady-state vmcnt
    # bookkeeping: iterations 0, 1 and >= 2 differ), ragged last column tiles, tanh; and the real 50x50 MNIST-U geometry
    (40, 28, 28, 8, 32, 8, 1, 1), (24, 64, 64, 16, 16, 8, 1, 1), (12, 50, 28, 8, 32, 8, 1, 1), (2, 50, 28, 8, 8, 4, 2, 1),
    (3, 28, 28, 8, 16, 8, 2, 1),
    # several input channels (they join the reduction of the spectral GEMM)
    (3, 28, 28, 8, 16, 8, 1, 3), (2, 20, 9, 2, 5, 4, 0, 2),
    # frames beyond the specialised transforms along w (Lh > 64 or Ho > 64): spectra in frequency blocks, generic
    # transforms -- the galaxy configuration's shape class (192-wide frame, 3 channels) at a small size
    (2, 96, 32, 16, 4, 4, 1, 2), (2, 128, 64, 32, 2, 16, 1, 3),
    # round 4: the spectral GEMM kernels of their own shape at their edges -- one image (a single 128-column panel, two k-steps
    # per reduction slice), 2 M = 512 / 1 024 rows; and the weight gradient's 192-column tiles on a 1 152-column problem
    # (galaxy frame, three channels) with 2 M = 512 rows
    (1, 64, 64, 16, 32, 8, 1, 1), (2, 64, 64, 16, 32, 16, 1, 1), (3, 128, 64, 32, 16, 16, 1, 3),
    # round 5, the short circular frame L = max(n + pad, k) rounded up to 4 (csrc/abi_conv_dft.hip: dft_plan): a filter longer
    # than n + pad (frame = k), no padding at all (frame = n), odd sizes whose rounding stops at n + 2 pad, padding >= k
    (3, 20, 40, 12, 4, 4, 1, 1), (2, 24, 9, 0, 4, 4, 0, 1), (2, 21, 7, 3, 4, 4, 1, 1), (2, 19, 5, 1, 4, 4, 1, 2),
    (2, 16, 6, 8, 4, 4, 0, 1)])
@pytest.mark.parametrize('nparts', [3, 2])
def test_conv1_dft_matches_fp64(B, n, k, pad, C, R, act, Cin, nparts):
    """Frequency-domain lifting convolution (DFT + batched split-pipe GEMM): fp32-level agreement with fp64, in the exact
    bf16 split (3 parts, six products) and in the h3 arithmetic (2 fp16 parts, three products)."""
    from tvae._lib import query
    if not query('tvae_conv1_dft_supported', B, Cin, n, k, pad, C, R):
        pytest.skip('geometry not handled by the frequency-domain path')
    y = torch.rand(B, Cin, n, n, generator=torch.Generator().manual_seed(1))
    bank = rnd(C * R, Cin * k * k, seed=2, scale=(Cin * k * k) ** -0.5)
    bias = rnd(C, seed=3, scale=0.1)
    Ho = n + 2 * pad - k + 1
    ref = F.conv2d(y.double(), bank.double().view(C * R, Cin, k, k), None, 1, pad).view(B, C, R, Ho, Ho) \
        + bias.double().view(1, C, 1, 1, 1)
    ref = act_ref(ref, act)
    at = torch.zeros(query('tvae_conv1_dft_at_floats', B, Cin, n, k, pad, C, R), device=dev())
    ws = torch.empty(query('tvae_conv1_dft_ws_floats', B, Cin, n, k, pad, C, R), device=dev())
    out = torch.empty(C, B * R * Ho * Ho, device=dev())
    call('tvae_conv1_fwd_dft', y.to(dev()), bank.to(dev()), bias.to(dev()), out, at, ws, ws.numel(), B, Cin, n, k, pad,
         C, R, act, SLOPE, nparts)
    got = out.view(C, B, R, Ho, Ho).permute(1, 0, 2, 3, 4)
    assert rel_err(got, ref) < GEMM_TOL['f32']
    g = rnd(B, C, R, Ho, Ho, seed=4)
    ref_g = torch.nn.grad.conv2d_weight(y.double(), (C * R, Cin, k, k), g.double().view(B, C * R, Ho, Ho), padding=pad)
    dpre = g.permute(1, 0, 2, 3, 4).contiguous().view(C, -1).to(dev())
    dbank = torch.empty(C * R, Cin * k * k, device=dev())
    dbias = torch.empty(C, device=dev())
    call('tvae_conv1_wgrad_dft', dpre, at, dbank, dbias, ws, ws.numel(), B, Cin, n, k, pad, C, R, nparts)
    assert rel_err(dbias, g.double().sum(dim=(0, 2, 3, 4))) < TOL
    assert rel_err(dbank.view(C * R, Cin, k, k), ref_g) < GEMM_TOL['f32']


# ---- frequency-domain lifting convolution at the edges of its kernel instances (tvae_conv1_dft_route) --------------------
# tests/test_host_cpu.py::test_conv1_dft_routes_fit_their_instances_and_are_covered_on_the_gpu sweeps every frame on the host and
# fails when a (step, instance, parts) it meets is reached by no geometry of this list.
DFT_ROUTE_GEOMETRIES = [      # (B, Cin, n, k, pad, C, R, act)
    # every transform instance (ring 1 .. 6, h3, wide, generic, fixed-size) at the smallest and the largest Ho and Lh it admits
    (2, 1, 30, 20, 3, 2, 4, 1), (2, 1, 74, 48, 3, 2, 4, 1), (2, 1, 54, 22, 3, 2, 4, 1), (2, 1, 38, 28, 3, 2, 4, 1),
    (2, 1, 90, 64, 3, 2, 4, 1), (2, 1, 64, 28, 1, 2, 4, 1), (2, 1, 122, 97, 3, 2, 4, 1), (2, 1, 8, 1, 68, 2, 4, 1),
    (2, 1, 9, 1, 28, 2, 4, 1), (2, 1, 171, 32, 2, 2, 4, 1), (2, 1, 8, 1, 76, 2, 4, 1), (2, 1, 159, 4, 2, 2, 4, 1),
    (2, 1, 9, 1, 68, 2, 4, 1), (2, 1, 90, 32, 3, 2, 4, 1), (2, 1, 158, 5, 3, 2, 4, 1), (2, 1, 187, 32, 2, 2, 4, 1),
    (2, 1, 170, 111, 3, 2, 4, 1), (2, 1, 8, 128, 60, 2, 4, 1), (2, 1, 207, 180, 2, 2, 4, 1), (2, 1, 170, 145, 3, 2, 4, 1),
    (2, 1, 122, 98, 3, 2, 4, 1), (2, 1, 122, 96, 3, 2, 4, 1), (2, 1, 122, 65, 3, 2, 4, 1), (2, 1, 229, 166, 0, 2, 4, 1),
    (2, 1, 170, 144, 3, 2, 4, 1), (2, 1, 170, 113, 3, 2, 4, 1), (2, 1, 122, 64, 3, 2, 4, 1), (2, 1, 186, 97, 3, 2, 4, 1),
    (2, 1, 242, 153, 3, 2, 4, 1), (2, 1, 170, 112, 3, 2, 4, 1), (2, 1, 186, 96, 3, 2, 4, 1), (2, 1, 186, 65, 3, 2, 4, 1),
    (2, 1, 256, 139, 5, 2, 4, 1), (2, 1, 186, 64, 3, 2, 4, 1), (2, 1, 186, 33, 3, 2, 4, 1), (2, 1, 256, 131, 17, 2, 4, 1),
    (2, 1, 8, 44, 18, 2, 4, 1), (2, 1, 38, 13, 3, 2, 4, 1), (2, 1, 45, 14, 0, 2, 4, 1), (2, 1, 38, 12, 3, 2, 4, 1),
    (2, 1, 45, 13, 0, 2, 4, 1), (2, 1, 38, 11, 3, 2, 4, 1), (2, 1, 18, 1, 23, 2, 4, 1), (2, 1, 38, 1, 3, 2, 4, 1),
    (2, 1, 45, 1, 0, 2, 4, 1), (2, 1, 8, 96, 44, 2, 4, 1), (2, 1, 90, 65, 3, 2, 4, 1), (2, 1, 97, 66, 0, 2, 4, 1),
    (2, 1, 97, 65, 0, 2, 4, 1), (2, 1, 90, 63, 3, 2, 4, 1), (2, 1, 90, 33, 3, 2, 4, 1), (2, 1, 97, 34, 0, 2, 4, 1),
    (2, 1, 8, 8, 0, 2, 4, 1), (2, 1, 8, 1, 12, 2, 4, 1), (2, 1, 8, 1, 0, 2, 4, 1), (2, 1, 123, 96, 2, 2, 4, 1),
    (2, 1, 9, 1, 12, 2, 4, 1), (2, 1, 123, 95, 2, 2, 4, 1), (2, 1, 8, 1, 13, 2, 4, 1), (2, 1, 8, 1, 28, 2, 4, 1),
    (2, 1, 123, 64, 2, 2, 4, 1), (2, 1, 8, 1, 62, 2, 4, 1), (2, 1, 171, 44, 2, 2, 4, 1), (2, 1, 86, 1, 7, 2, 4, 1),
    (2, 1, 57, 1, 4, 2, 4, 1), (2, 1, 247, 152, 2, 2, 4, 1), (2, 1, 170, 77, 3, 2, 4, 1), (2, 1, 85, 1, 8, 2, 4, 1),
    (2, 1, 118, 1, 7, 2, 4, 1), (2, 1, 251, 124, 2, 2, 4, 1), (2, 1, 170, 76, 3, 2, 4, 1), (2, 1, 170, 45, 3, 2, 4, 1),
    (2, 1, 117, 1, 8, 2, 4, 1), (2, 1, 90, 1, 35, 2, 4, 1), (2, 1, 251, 96, 2, 2, 4, 1), (2, 1, 250, 148, 3, 2, 4, 1),
    (2, 1, 9, 1, 62, 2, 4, 1), (2, 1, 38, 27, 3, 2, 4, 1), (2, 1, 45, 28, 0, 2, 4, 1), (2, 1, 8, 1, 5, 2, 4, 1),
    (2, 1, 59, 46, 2, 2, 4, 1), (2, 1, 97, 64, 0, 2, 4, 1), (2, 1, 8, 64, 28, 2, 4, 1), (2, 1, 9, 1, 5, 2, 4, 1),
    (2, 1, 123, 94, 2, 2, 4, 1), (2, 1, 9, 1, 13, 2, 4, 1),
    # Ho = 32 j, 32 j + 1, 32 j + 31 (whole, one-column and one-short output tiles), tanh at the last
    (2, 1, 8, 1, 44, 2, 4, 1), (2, 1, 8, 1, 60, 2, 4, 1), (2, 1, 9, 1, 44, 2, 4, 1), (2, 1, 9, 1, 60, 2, 4, 1),
    (2, 1, 9, 1, 11, 2, 4, 2), (2, 1, 9, 1, 27, 2, 4, 2), (2, 1, 9, 1, 43, 2, 4, 2), (2, 1, 9, 1, 59, 2, 4, 2),
    (2, 1, 9, 1, 75, 2, 4, 2),
    # the h3 frames around the dY instance's staging bound (32 Ho <= 11 * 64 * 6: Ho <= 132) and the end of its tables (Ho 144),
    # among them the galaxy frame with two more pixels of padding (n 128, k 64, pad 34: Ho 133) and n 128, k 20, pad 16 (Ho 141)
    (2, 1, 9, 1, 66, 2, 4, 1), (2, 1, 128, 64, 34, 2, 4, 1), (2, 1, 128, 20, 16, 2, 4, 1),
    # Lh = 64 / 65, 82 / 83, 88 / 89, 96 / 97: the register slots of the wide and the h3 instances, no activation
    (2, 1, 124, 1, 1, 2, 4, 0), (2, 1, 122, 1, 3, 2, 4, 0), (2, 1, 160, 3, 1, 2, 4, 0), (2, 1, 158, 5, 3, 2, 4, 0),
    (2, 1, 172, 15, 1, 2, 4, 0), (2, 1, 170, 17, 3, 2, 4, 0), (2, 1, 188, 31, 1, 2, 4, 0), (2, 1, 186, 161, 3, 2, 4, 0),
    # B Ho = 126 and 129: just below and just above the 128-column panel (NBpad)
    (3, 1, 8, 1, 17, 2, 4, 1), (3, 1, 9, 1, 17, 2, 4, 1),
    # three input channels on the wide frames
    (2, 3, 9, 1, 28, 2, 4, 1), (2, 3, 158, 5, 3, 2, 4, 1), (2, 3, 57, 1, 4, 2, 4, 1), (2, 3, 85, 1, 8, 2, 4, 1),
    (2, 3, 117, 1, 8, 2, 4, 1),
    # the spectral GEMM forms: panel resident in LDS (2 M = 512 at 8 / 10 / 12 k-steps), 512-row tile (2 k Cin > 256),
    # the exact-fit weight-gradient tile (2 M = 256, 2 k Cin > 128)
    (2, 1, 60, 60, 6, 32, 8, 1), (2, 1, 64, 76, 16, 32, 8, 1), (2, 3, 28, 30, 8, 32, 8, 1), (2, 3, 50, 44, 6, 2, 4, 1),
    (2, 3, 28, 28, 8, 16, 8, 1),
]
DFT_EDGE_GEOMETRIES = [       # one geometry per transform instance that h3 (parts = 2) reaches; no activation
    (2, 1, 30, 20, 3, 2, 4, 0), (2, 1, 74, 48, 3, 2, 4, 0), (2, 1, 54, 22, 3, 2, 4, 0), (2, 1, 38, 28, 3, 2, 4, 0),
    (2, 1, 90, 64, 3, 2, 4, 0), (2, 1, 64, 28, 1, 2, 4, 0), (2, 1, 122, 97, 3, 2, 4, 0), (2, 1, 8, 1, 76, 2, 4, 0),
    (2, 1, 158, 5, 3, 2, 4, 0), (2, 1, 8, 128, 60, 2, 4, 0), (2, 1, 229, 166, 0, 2, 4, 0), (2, 1, 186, 97, 3, 2, 4, 0),
    (2, 1, 186, 96, 3, 2, 4, 0), (2, 1, 186, 64, 3, 2, 4, 0), (2, 1, 8, 44, 18, 2, 4, 0), (2, 1, 38, 12, 3, 2, 4, 0),
    (2, 1, 38, 11, 3, 2, 4, 0), (2, 1, 8, 96, 44, 2, 4, 0), (2, 1, 97, 65, 0, 2, 4, 0), (2, 1, 90, 63, 3, 2, 4, 0),
    (2, 1, 8, 8, 0, 2, 4, 0), (2, 1, 9, 1, 12, 2, 4, 0), (2, 1, 8, 1, 13, 2, 4, 0), (2, 1, 170, 111, 3, 2, 4, 0),
    (2, 1, 186, 65, 3, 2, 4, 0), (2, 1, 171, 32, 2, 2, 4, 0), (2, 1, 8, 1, 68, 2, 4, 0), (2, 1, 38, 13, 3, 2, 4, 0),
    (2, 1, 18, 1, 23, 2, 4, 0),
]


def dft_fp64(y, bank, bias, g, k, pad, act):
    """fp64 references of the lifting convolution (out, act applied), its weight gradient and its bias gradient for the output
    gradient g [B][C][R][Ho][Ho]: plain F.conv2d / conv2d_weight in float64 (on the GPU: the largest frames here have 180-tap
    filters whose unfolded operand does not fit a host test)."""
    B, Cin = y.shape[:2]
    CR, C = bank.shape[0], bias.shape[0]
    yd, wd = y.double().to(dev()), bank.double().to(dev()).view(CR, Cin, k, k)
    pre = F.conv2d(yd, wd, None, 1, pad)
    Ho = pre.shape[-1]
    out = act_ref(pre.view(B, C, CR // C, Ho, Ho) + bias.double().to(dev()).view(1, C, 1, 1, 1), act)
    gd = g.double().to(dev())
    dbank = torch.nn.grad.conv2d_weight(yd, (CR, Cin, k, k), gd.view(B, CR, Ho, Ho), padding=pad)
    return out.cpu(), dbank.cpu(), gd.sum(dim=(0, 2, 3, 4)).cpu()


def dft_run(y, bank, bias, dpre, B, Cin, n, k, pad, C, R, act, parts):
    """Forward and weight gradient through the C ABI; returns out [B][C][R][Ho][Ho], dbank, dbias and A^T with its trailer.
    Outputs start as NaN: an element no kernel writes fails the comparison."""
    Ho = n + 2 * pad - k + 1
    at = torch.zeros(query('tvae_conv1_dft_at_floats', B, Cin, n, k, pad, C, R), device=dev())
    ws = torch.empty(query('tvae_conv1_dft_ws_floats', B, Cin, n, k, pad, C, R), device=dev())
    out = torch.full((C, B * R * Ho * Ho), float('nan'), device=dev())
    call('tvae_conv1_fwd_dft', y.to(dev()), bank.to(dev()), bias.to(dev()), out, at, ws, ws.numel(), B, Cin, n, k, pad, C, R,
         act, SLOPE, parts)
    dbank = torch.full((C * R, Cin * k * k), float('nan'), device=dev())
    dbias = torch.full((C,), float('nan'), device=dev())
    call('tvae_conv1_wgrad_dft', dpre.to(dev()), at, dbank, dbias, ws, ws.numel(), B, Cin, n, k, pad, C, R, parts)
    torch.cuda.synchronize()
    return out.view(C, B, R, Ho, Ho).permute(1, 0, 2, 3, 4).cpu(), dbank.cpu(), dbias.cpu(), at.cpu()


@pytest.mark.parametrize('B,Cin,n,k,pad,C,R,act', DFT_ROUTE_GEOMETRIES)
def test_conv1_dft_route_edges(B, Cin, n, k, pad, C, R, act):
    """Every instance of the transforms along w and of the spectral GEMMs at the edges of the frames it is routed, against fp64:
    the exact three-part split and h3 to 2e-5 (as test_conv1_dft_matches_fp64), the one-part bf16 mode to 1.5e-2 (as
    test_conv1_dft_bf16_mode).  Each fp64 reference is computed once for the three arithmetics."""
    assert query('tvae_conv1_dft_supported', B, Cin, n, k, pad, C, R)
    Ho = n + 2 * pad - k + 1
    y = torch.rand(B, Cin, n, n, generator=torch.Generator().manual_seed(1))
    bank = rnd(C * R, Cin * k * k, seed=2, scale=(Cin * k * k) ** -0.5)
    bias = rnd(C, seed=3, scale=0.1)
    g = rnd(B, C, R, Ho, Ho, seed=4)
    ref, ref_g, ref_db = dft_fp64(y, bank, bias, g, k, pad, act)
    dpre = g.permute(1, 0, 2, 3, 4).contiguous().view(C, -1)
    for parts in (3, 2, 1):
        tol = GEMM_TOL['f32'] if parts > 1 else 1.5e-2
        routes = [query('tvae_conv1_dft_route', B, Cin, n, k, pad, C, R, parts, w) for w in range(4)]
        got, dbank, dbias, _ = dft_run(y, bank, bias, dpre, B, Cin, n, k, pad, C, R, act, parts)
        assert rel_err(got, ref) < tol, (parts, routes, rel_err(got, ref))
        assert rel_err(dbank.view(C * R, Cin, k, k), ref_g) < tol, (parts, routes, rel_err(dbank.view(C * R, Cin, k, k), ref_g))
        assert rel_err(dbias, ref_db) < (TOL if parts > 1 else tol), (parts, routes, rel_err(dbias, ref_db))


def test_conv1_dft_first_unsupported_geometry_launches_nothing():
    """Ho = 161 (six 32-row output tiles, one more than any instance takes): both entry points refuse it, in every arithmetic,
    and leave the output, A^T and the workspace as they were."""
    from tvae._lib import TvaeHipError
    B, Cin, n, k, pad, C, R = 2, 1, 9, 1, 76, 2, 4
    Ho = n + 2 * pad - k + 1
    assert Ho == 161 and query('tvae_conv1_dft_supported', B, Cin, n, k, pad - 1, C, R)
    assert not query('tvae_conv1_dft_supported', B, Cin, n, k, pad, C, R)
    y, bank, bias = torch.rand(B, Cin, n, n, device=dev()), torch.rand(C * R, k * k, device=dev()), torch.zeros(C, device=dev())
    at = torch.full((max(query('tvae_conv1_dft_at_floats', B, Cin, n, k, pad, C, R), 4096),), 7.0, device=dev())
    ws = torch.full((max(query('tvae_conv1_dft_ws_floats', B, Cin, n, k, pad, C, R), 4096),), 7.0, device=dev())
    out = torch.full((C, B * R * Ho * Ho), 7.0, device=dev())
    dbank, dbias = torch.full((C * R, k * k), 7.0, device=dev()), torch.full((C,), 7.0, device=dev())
    for parts in (1, 2, 3):
        assert all(query('tvae_conv1_dft_route', B, Cin, n, k, pad, C, R, parts, w) == -1 for w in range(4))
        with pytest.raises(TvaeHipError):
            call('tvae_conv1_fwd_dft', y, bank, bias, out, at, ws, ws.numel(), B, Cin, n, k, pad, C, R, 1, SLOPE, parts)
        with pytest.raises(TvaeHipError):
            call('tvae_conv1_wgrad_dft', out, at, dbank, dbias, ws, ws.numel(), B, Cin, n, k, pad, C, R, parts)
    torch.cuda.synchronize()
    for t in (at, ws, out, dbank, dbias):
        assert bool((t == 7.0).all())


@pytest.mark.parametrize('B,Cin,n,k,pad,C,R,act', DFT_EDGE_GEOMETRIES)
def test_conv1_dft_h3_edge_placed_maxima(B, Cin, n, k, pad, C, R, act):
    """h3 (parts = 2) on one geometry per transform instance, with the largest input values where tiles end: a 2^8 spike at
    the last pixel of the last image and channel, and in the output gradient at the last w of the last row of the last image
    and at the first column of the second 32-column tile.  Per-row accuracy against fp64 (rows of out: (image, filter);
    of dbank: filter rows); the per-channel maxima behind A^T equal max |out| exactly; every operand maximum the kernels
    leave behind A^T (cmax [Lh][B], fmax [Lh], wmax [Lh][2 M of Mb], smax [M]) is finite and positive.
    No activation: the transforms along w spread an error of ~1e-7 of the spike's pre-activation value over its output row,
    in every arithmetic (parts = 3 as well); a LeakyReLU that shrinks a negative spike 100-fold leaves that error in place
    against a row norm 100 times smaller (1.2e-5 per row at Ho = 160) -- a property of the frequency-domain form, not of the
    maxima this test is about."""
    Ho = n + 2 * pad - k + 1
    y = torch.rand(B, Cin, n, n, generator=torch.Generator().manual_seed(1))
    y[-1, -1, -1, -1] = 2.0 ** 8
    bank = rnd(C * R, Cin * k * k, seed=2, scale=(Cin * k * k) ** -0.5)
    bias = rnd(C, seed=3, scale=0.1)
    g = rnd(B, C, R, Ho, Ho, seed=4)
    g[-1, -1, -1, -1, -1] = 2.0 ** 8
    if B * Ho > 32:                                       # column (image, row) 32: the seam of the first two tiles
        g[32 // Ho, 0, 0, 32 % Ho, Ho - 1] = -2.0 ** 8
    ref, ref_g, ref_db = dft_fp64(y, bank, bias, g, k, pad, act)
    dpre = g.permute(1, 0, 2, 3, 4).contiguous().view(C, -1)
    got, dbank, dbias, at = dft_run(y, bank, bias, dpre, B, Cin, n, k, pad, C, R, act, 2)
    routes = [query('tvae_conv1_dft_route', B, Cin, n, k, pad, C, R, 2, w) for w in range(2)]
    assert row_rel_err(got.reshape(B * C * R, -1), ref.reshape(B * C * R, -1)) < ROW_TOL, routes
    assert row_rel_err(dbank, ref_g.reshape(C * R, -1)) < ROW_TOL, routes
    assert rel_err(dbias, ref_db) < TOL, routes
    # trailer of A^T (csrc/abi_conv_dft.hip: DftPlan): cmax, fmax, wmax, smax, then the per-channel maxima as its last C words
    Lh = query('tvae_conv1_dft_frame', B, Cin, n, k, pad, C, R) // 2 + 1
    M, K2, NBpad, Mb = C * R, 2 * k * Cin, -(-B * Ho // 128) * 128, -(-2 * C * R // 512) * 512
    base = (Lh * K2 * NBpad + 3) // 4 * 4
    o_fmax, o_wmax = Lh * B, Lh * B + Lh
    o_smax = o_wmax + Lh * Mb
    assert at.numel() == base + (o_smax + M + 3) // 4 * 4 + C
    assert torch.equal(at[-C:], got.abs().amax(dim=(0, 2, 3, 4))), routes
    tr = at[base:]
    for name, words in (('cmax', tr[:o_fmax]), ('fmax', tr[o_fmax:o_wmax]),
                        ('wmax', tr[o_wmax:o_smax].view(Lh, Mb)[:, :2 * M]), ('smax', tr[o_smax:o_smax + M])):
        assert bool(torch.isfinite(words).all()) and bool((words > 0).all()), (name, routes, words.min())



@pytest.mark.parametrize('B,n,k,pad,C,R,act', [
    (24, 64, 64, 16, 16, 8, 1), (40, 28, 28, 8, 32, 8, 1), (12, 50, 28, 8, 32, 8, 2),      # ring frames: bf16 STORAGE of T and S'
    (5, 40, 32, 6, 64, 4, 0), (3, 28, 28, 8, 16, 8, 1)])                                  # register-staged frame; ragged ring batch
def test_conv1_dft_bf16_mode(B, n, k, pad, C, R, act):
    """The one-part bf16 throughput mode of the frequency-domain convolution (parts = 1; never fp32-equivalent): operands
    rounded to bf16 and, on the ring frames, T and S' STORED as bf16 (round 4).  Own tolerance: 1.5e-2 relative Frobenius
    against fp64 for the output and the weight gradient (the exact modes hold 2e-5 on the same geometries)."""
    from tvae._lib import query
    Cin = 1
    y = torch.rand(B, Cin, n, n, generator=torch.Generator().manual_seed(1))
    bank = rnd(C * R, Cin * k * k, seed=2, scale=(Cin * k * k) ** -0.5)
    bias = rnd(C, seed=3, scale=0.1)
    Ho = n + 2 * pad - k + 1
    ref = act_ref(F.conv2d(y.double(), bank.double().view(C * R, Cin, k, k), None, 1, pad).view(B, C, R, Ho, Ho)
                  + bias.double().view(1, C, 1, 1, 1), act)
    at = torch.zeros(query('tvae_conv1_dft_at_floats', B, Cin, n, k, pad, C, R), device=dev())
    ws = torch.empty(query('tvae_conv1_dft_ws_floats', B, Cin, n, k, pad, C, R), device=dev())
    out = torch.full((C, B * R * Ho * Ho), float('nan'), device=dev())
    call('tvae_conv1_fwd_dft', y.to(dev()), bank.to(dev()), bias.to(dev()), out, at, ws, ws.numel(), B, Cin, n, k, pad, C, R, act,
         SLOPE, 1)
    got = out.view(C, B, R, Ho, Ho).permute(1, 0, 2, 3, 4)
    assert torch.isfinite(got).all()
    assert rel_err(got, ref) < 1.5e-2
    g = rnd(B, C, R, Ho, Ho, seed=4)
    ref_g = torch.nn.grad.conv2d_weight(y.double(), (C * R, Cin, k, k), g.double().view(B, C * R, Ho, Ho), padding=pad)
    dpre = g.permute(1, 0, 2, 3, 4).contiguous().view(C, -1).to(dev())
    dbank = torch.full((C * R, Cin * k * k), float('nan'), device=dev())
    dbias = torch.empty(C, device=dev())
    call('tvae_conv1_wgrad_dft', dpre, at, dbank, dbias, ws, ws.numel(), B, Cin, n, k, pad, C, R, 1)
    assert torch.isfinite(dbank).all()
    assert rel_err(dbank.view(C * R, Cin, k, k), ref_g) < 1.5e-2
    assert rel_err(dbias, g.double().sum(dim=(0, 2, 3, 4))) < 1.5e-2


@pytest.mark.parametrize('F_,B,Np,M,act', [(512, 3, 256, 512, 1), (300, 2, 384, 512, 1), (64, 2, 128, 200, 2)])
def test_linear_dgrad_x6_fused_first_layer(F_, B, Np, M, act):
    """Data gradient of the first hidden layer fused with the backward of the coordinate layer: dX is never stored."""
    from tvae._lib import query
    Nt = B * Np
    W, d = rnd(M, F_, seed=1, scale=M ** -0.5), rnd(M, Nt, seed=2)
    aux = rnd(F_, Nt, seed=3).clamp(-0.9, 0.9)
    xr, Wc = rnd(Nt, 2, seed=4), rnd(F_, 2, seed=5)
    d0 = (W.double().t() @ d.double()) * dact_ref(aux.double(), act)
    w3t = torch.empty(query('tvae_dense_x6_bytes', F_, M) // 4, device=dev())
    call('tvae_dense_split3', W.to(dev()), F_, w3t, w3t.numel() * 4, F_, M, 1, None, None)
    gxr = torch.empty(Nt, 2, device=dev())
    part = torch.empty((Nt // 128) * F_ * 3, device=dev())
    call('tvae_linear_dgrad_x6', w3t, d.to(dev()), None, aux.to(dev()), None, M, Nt, F_, Nt, Nt, act, SLOPE, in_xr=xr.to(dev()),
         in_wc=Wc.to(dev()), in_gxr=gxr, in_part=part, in_part_floats=part.numel(), parts=3)
    Simg = torch.empty(B, F_, device=dev())
    dbc = torch.empty(F_, device=dev())
    dWc = torch.empty(F_, 2, device=dev())
    call('tvae_dec_in_total', part, B, Np // 128, F_, Simg, dbc, dWc)
    assert rel_err(gxr, d0.t() @ Wc.double()) < GEMM_TOL['f32']
    assert rel_err(Simg, d0.view(F_, B, Np).sum(2).t()) < GEMM_TOL['f32']
    assert rel_err(dbc, d0.sum(1)) < GEMM_TOL['f32']
    assert rel_err(dWc, d0 @ xr.double()) < GEMM_TOL['f32']


def test_linear_x6_implicit_gradient_operand():
    """dgrad / wgrad with the gradient operand formed on the fly from (Wo, gy, saved activation)."""
    from tvae._lib import query
    M, N, K = 512, 1024, 512
    W, H = rnd(M, K, seed=1, scale=M ** -0.5), rnd(M, N, seed=2).clamp(-0.9, 0.9)
    wo, gy = rnd(M, seed=3), rnd(N, seed=4)
    aux, X = rnd(K, N, seed=5).clamp(-0.9, 0.9), rnd(K, N, seed=6)
    d = wo.double()[:, None] * gy.double()[None, :] * dact_ref(H.double(), 1)
    w3t = torch.empty(query('tvae_dense_x6_bytes', K, M) // 4, device=dev())
    call('tvae_dense_split3', W.to(dev()), K, w3t, w3t.numel() * 4, K, M, 1, None, None)
    dX = torch.empty(K, N, device=dev())
    call('tvae_linear_dgrad_x6', w3t, H.to(dev()), None, aux.to(dev()), dX, M, N, K, N, N, 1, SLOPE, vg_wo=wo.to(dev()),
         vg_gy=gy.to(dev()), parts=3)
    assert rel_err(dX, (W.double().t() @ d) * dact_ref(aux.double(), 1)) < GEMM_TOL['f32']
    # the same product in the two-valued form (LeakyReLU): weights scaled by wo before the split, 0 / 1 streamed operand
    csum = torch.empty(K, device=dev())
    call('tvae_dense_split3', W.to(dev()), K, w3t, w3t.numel() * 4, K, M, 1, wo.to(dev()), csum)
    assert rel_err(csum, (W.double() * wo.double()[:, None]).sum(0)) < TOL
    dX2 = torch.empty(K, N, device=dev())
    call('tvae_linear_dgrad_x6', w3t, H.to(dev()), None, aux.to(dev()), dX2, M, N, K, N, N, 1, SLOPE, vg_gy=gy.to(dev()),
         vg_csum=csum, parts=3)
    assert rel_err(dX2, (W.double().t() @ d) * dact_ref(aux.double(), 1)) < GEMM_TOL['f32']
    # ... and with the row sums of the streamed activation against gy (ABI 3: what tvae_dec_out_bwd computes in a pass of its
    # own): the data gradient is bitwise the same launch result, db / dwo agree with fp64
    for Mr in (512, 384):
        Hr, wor = H[:Mr].contiguous(), wo[:Mr].contiguous()
        w3r = torch.empty(query('tvae_dense_x6_bytes', K, Mr) // 4, device=dev())
        csr = torch.empty(K, device=dev())
        call('tvae_dense_split3', W[:Mr].contiguous().to(dev()), K, w3r, w3r.numel() * 4, K, Mr, 1, wor.to(dev()), csr)
        dXa, dXb = torch.empty(K, N, device=dev()), torch.empty(K, N, device=dev())
        call('tvae_linear_dgrad_x6', w3r, Hr.to(dev()), None, aux.to(dev()), dXa, Mr, N, K, N, N, 1, SLOPE, vg_gy=gy.to(dev()),
             vg_csum=csr, parts=3)
        rs_part = torch.full(((N // 128) * Mr * 2,), float('nan'), device=dev())
        gys = gy.sum().reshape(1).to(dev())
        rs_db, rs_dwo = torch.empty(Mr, device=dev()), torch.empty(Mr, device=dev())
        call('tvae_linear_dgrad_x6', w3r, Hr.to(dev()), None, aux.to(dev()), dXb, Mr, N, K, N, N, 1, SLOPE, vg_gy=gy.to(dev()),
             vg_csum=csr, rs_part=rs_part, rs_part_floats=rs_part.numel(), rs_wo=wor.to(dev()), rs_gysum=gys, rs_db=rs_db,
             rs_dwo=rs_dwo, parts=3)
        assert torch.equal(dXa, dXb)
        assert rel_err(rs_db, (wor.double()[:, None] * gy.double()[None, :] * dact_ref(Hr.double(), 1)).sum(1)) < TOL
        assert rel_err(rs_dwo, Hr.double() @ gy.double()) < TOL
    with pytest.raises(Exception):         # the row sums need the two-valued form (csum) and a workspace of N/128 * M * 2
        call('tvae_linear_dgrad_x6', w3t, H.to(dev()), None, aux.to(dev()), dX2, M, N, K, N, N, 1, SLOPE, vg_gy=gy.to(dev()),
             vg_csum=csum, rs_part=rs_part, rs_part_floats=16, rs_wo=wo.to(dev()), rs_gysum=gys, rs_db=rs_db, rs_dwo=rs_dwo,
             parts=3)
    # packed sign bits of the activation (the weight gradient below can read its 0 / 1 operand from them)
    def pack_bits(t):                      # bit (n & 31) of word n / 32 = [t[m][n] > 0]
        b = (t > 0).to(torch.int64).view(t.shape[0], -1, 32)
        w = (b << torch.arange(32)).sum(-1)
        return (w - ((w >> 31) << 32)).to(torch.int32).contiguous()
    hb = pack_bits(H).to(dev())
    with pytest.raises(Exception):         # the two-valued form exists for LeakyReLU only
        call('tvae_linear_dgrad_x6', w3t, H.to(dev()), None, aux.to(dev()), dX2, M, N, K, N, N, 2, SLOPE, vg_gy=gy.to(dev()),
             vg_csum=csum, parts=3)
    ws = torch.empty(1 << 26, device=dev())       # >= tvae_linear_wgrad_x6_ws_floats(M, N, K): slices x M x K
    for vact in (1, 2):                    # LeakyReLU: two-valued weight gradient; tanh: generic implicit operand
        dv = wo.double()[:, None] * gy.double()[None, :] * dact_ref(H.double(), vact)
        dW = torch.empty(M, K, device=dev())
        call('tvae_linear_wgrad_x6', H.to(dev()), X.to(dev()), dW, ws, ws.numel(), M, N, K, N, N, 0, vg_wo=wo.to(dev()),
             vg_gy=gy.to(dev()), vg_act=vact, vg_slope=SLOPE, parts=3)
        assert rel_err(dW, dv @ X.double().t()) < GEMM_TOL['f32'], vact
        if vact == 1:                      # the same from the packed sign bits: bitwise the same sums
            dWb = torch.empty(M, K, device=dev())
            call('tvae_linear_wgrad_x6', None, X.to(dev()), dWb, ws, ws.numel(), M, N, K, N, N, 0, vg_wo=wo.to(dev()),
                 vg_gy=gy.to(dev()), vg_act=1, vg_slope=SLOPE, vg_bits=hb, parts=3)
            assert torch.equal(dWb, dW)
    # a LeakyReLU forward launch stores the sign bits of its output
    w3 = torch.empty(query('tvae_dense_x6_bytes', M, K) // 4, device=dev())
    call('tvae_dense_split3', W.to(dev()), K, w3, w3.numel() * 4, M, K, 0, None, None)
    Y = torch.empty(M, N, device=dev())
    yb = torch.empty(M, N // 32, dtype=torch.int32, device=dev())
    call('tvae_linear_fwd_x6', w3, X.to(dev()), None, None, Y, M, N, K, N, N, 1, SLOPE, sign_bits=yb, parts=3)
    assert torch.equal(yb.cpu(), pack_bits(Y.cpu()))
    # dec_out_bwd without the gradient tensor: sums only
    F_ = M
    part = torch.empty(((N + 1023) // 1024) * F_ * 2, device=dev())
    tot = torch.empty(2, F_, device=dev())
    call('tvae_dec_out_bwd', gy.view(N, 1).to(dev()), 1, wo.view(1, F_).to(dev()), H.to(dev()), N, None, N, F_, N, 1,
         SLOPE, part, part.numel(), tot)
    assert rel_err(tot[0], d.sum(1)) < TOL and rel_err(tot[1], H.double() @ gy.double()) < TOL


@pytest.mark.parametrize('sw,sg,sx', [(1.0, 1.0, 1.0), (1e-3, 1e-6, 1.0), (30.0, 1e3, 50.0), (1.0, 0.0, 1.0), (1e-12, 1e-9, 1e-3)])
def test_h3_decoder_entry_points(sw, sg, sx):
    """The three decoder launches with an h3 instance (two fp16 parts per operand under a power-of-two tensor scale: three
    products per block, two against the exact 0 / 1 operand) against fp64 at the fp32 tolerance, and against the exact x6
    split of the same launch: forward with the recomputed first-layer operand (+ sign bits), two-valued data gradient (+ row
    sums), weight gradient from sign bits against gy x the recomputed operand.  Operand magnitudes from 1e-12 to 1e3 (the
    scales must absorb them: fp16 alone spans 6e-8 .. 6.5e4), a zero gradient (maximum 0)."""
    from tvae._lib import query
    F_, B, Np, M, act = 512, 2, 256, 512, 1
    Nt = B * Np
    xr, Wc, bc = (rnd(Nt, 2, seed=1) * sx).to(dev()), rnd(F_, 2, seed=2).to(dev()), rnd(F_, seed=3).to(dev())
    LB = rnd(B, F_, seed=4).to(dev())
    h0 = torch.empty(F_, Nt, device=dev())
    call('tvae_dec_l0_fwd', xr, Wc, bc, LB, h0, Nt, F_, Nt, Np, act, SLOPE)
    W, b = rnd(M, F_, seed=5, scale=sw * F_ ** -0.5), rnd(M, seed=6, scale=sw)
    wo, gy = rnd(M, seed=8), rnd(Nt, seed=9) * sg
    va = dict(va_xr=xr, va_wc=Wc, va_bc=bc, va_lb=LB, va_np=Np)
    H0 = h0.double().cpu()
    res = {}
    for nparts, split in ((3, 'tvae_dense_split3'), (2, 'tvae_dense_split2h')):
        w3 = torch.empty(query('tvae_dense_x6_bytes', M, F_) // 4, device=dev())
        call(split, W.to(dev()), F_, w3, w3.numel() * 4, M, F_, 0, None, None)
        Y = torch.empty(M, Nt, device=dev())
        bits = torch.empty(M, Nt // 32, dtype=torch.int32, device=dev())
        call('tvae_linear_fwd_x6', w3, None, b.to(dev()), None, Y, M, Nt, F_, Nt, Nt, act, SLOPE, **va, sign_bits=bits,
             parts=nparts)
        # two-valued data gradient of THIS layer's input from (wo, gy, Y): weights W^T diag(wo), 0 / 1 operand [Y > 0]
        w3t = torch.empty(query('tvae_dense_x6_bytes', F_, M) // 4, device=dev())
        csum = torch.empty(F_, device=dev())
        call(split, W.to(dev()), F_, w3t, w3t.numel() * 4, F_, M, 1, wo.to(dev()), csum)
        dX = torch.empty(F_, Nt, device=dev())
        rs_part = torch.full(((Nt // 128) * M * 2,), float('nan'), device=dev())
        gys = gy.sum().reshape(1).to(dev())
        rs_db, rs_dwo = torch.empty(M, device=dev()), torch.empty(M, device=dev())
        call('tvae_linear_dgrad_x6', w3t, Y, None, h0, dX, M, Nt, F_, Nt, Nt, 1, SLOPE, vg_gy=gy.to(dev()), vg_csum=csum,
             rs_part=rs_part, rs_part_floats=rs_part.numel(), rs_wo=wo.to(dev()), rs_gysum=gys, rs_db=rs_db, rs_dwo=rs_dwo,
             parts=nparts)
        ws = torch.empty(query('tvae_linear_wgrad_x6_ws_floats', M, Nt, F_), device=dev())
        dW = torch.empty(M, F_, device=dev())
        call('tvae_linear_wgrad_x6', None, None, dW, ws, ws.numel(), M, Nt, F_, Nt, Nt, 0, vg_wo=wo.to(dev()),
             vg_gy=gy.to(dev()), vg_act=1, vg_slope=SLOPE, **va, vg_bits=bits, parts=nparts)
        res[nparts] = (Y, dX, dW, rs_db, rs_dwo, bits)
        assert torch.isfinite(Y).all() and torch.isfinite(dX).all() and torch.isfinite(dW).all()
    Yd = res[3][0].double().cpu()                     # masks from the x6 forward (the two forwards may differ in a sign at 0)
    ref_Y = act_ref(W.double() @ H0 + b.double()[:, None], act)
    d = wo.double()[:, None] * gy.double()[None, :] * dact_ref(Yd, 1)
    ref_dX = (W.double().t() @ d) * dact_ref(H0, 1)
    ref_dW = d @ H0.t()
    flips = int(((res[2][0] > 0) != (res[3][0] > 0)).sum())
    assert flips <= 2                                 # elements at zero to rounding
    for nparts in (3, 2):
        Y, dX, dW, rs_db, rs_dwo, bits = res[nparts]
        assert rel_err(Y, ref_Y) < GEMM_TOL['f32'], nparts
        if sg == 0.0:
            assert float(dX.abs().max()) == 0.0 and float(dW.abs().max()) == 0.0
            continue
        tol = GEMM_TOL['f32'] * (1 if (nparts == 3 or flips == 0) else 50)
        assert rel_err(dX, ref_dX) < tol, nparts
        assert rel_err(dW, ref_dW) < tol, nparts
    # h3 is not less accurate than the exact split by more than rounding (both are dominated by fp32 accumulation)
    e3, e2 = rel_err(res[3][0], ref_Y), rel_err(res[2][0], ref_Y)
    assert e2 < 2 * e3 + 1e-7, (e2, e3)
    # the recomputed operand with tanh (its bound |act(pre)| <= |pre| holds for every activation of the reference); unit scales
    # only: a saturated tanh of a difference of large terms is ill-conditioned in every arithmetic
    if (sw, sg, sx) != (1.0, 1.0, 1.0):
        return
    h0t = torch.empty(F_, Nt, device=dev())
    call('tvae_dec_l0_fwd', xr, Wc, bc, LB, h0t, Nt, F_, Nt, Np, 2, SLOPE)
    w3h = torch.empty(query('tvae_dense_x6_bytes', M, F_) // 4, device=dev())
    call('tvae_dense_split2h', W.to(dev()), F_, w3h, w3h.numel() * 4, M, F_, 0, None, None)
    Yt = torch.empty(M, Nt, device=dev())
    call('tvae_linear_fwd_x6', w3h, None, b.to(dev()), None, Yt, M, Nt, F_, Nt, Nt, 2, SLOPE, va_xr=xr, va_wc=Wc, va_bc=bc,
         va_lb=LB, va_np=Np, parts=2)
    assert rel_err(Yt, act_ref(W.double() @ h0t.double().cpu() + b.double()[:, None], 2)) < GEMM_TOL['f32']


@pytest.mark.parametrize('slack', [1.0, 256.0])
def test_linear_x6_h3_memory_operand_bounds(slack):
    """h3 (parts = 2) with the streamed operand READ FROM MEMORY under a caller-supplied bound (ABI 5: x_amax / a_amax): forward,
    plain data gradient and plain weight gradient against fp64 at the fp32 tolerance, with the exact maximum and with a bound
    2^8 too large (a loose bound costs head room, not correctness: include/tvae_hip.h)."""
    from tvae._lib import query
    M, N, K = 512, 1024, 384
    W, X, b = rnd(M, K, seed=1, scale=K ** -0.5), rnd(K, N, seed=2), rnd(M, seed=3)
    w3 = torch.empty(query('tvae_dense_x6_bytes', M, K) // 4, device=dev())
    call('tvae_dense_split2h', W.to(dev()), K, w3, w3.numel() * 4, M, K, 0, None, None)
    xmax = (X.abs().max() * slack).reshape(1).to(dev())
    Y = torch.full((M, N), float('nan'), device=dev())
    call('tvae_linear_fwd_x6', w3, X.to(dev()), b.to(dev()), None, Y, M, N, K, N, N, 1, SLOPE, parts=2, x_amax=xmax)
    assert rel_err(Y, act_ref(W.double() @ X.double() + b.double()[:, None], 1)) < GEMM_TOL['f32']
    with pytest.raises(Exception):                       # h3 with an operand from memory needs its bound
        call('tvae_linear_fwd_x6', w3, X.to(dev()), b.to(dev()), None, Y, M, N, K, N, N, 1, SLOPE, parts=2)
    # plain data gradient dX = W^T d
    d = rnd(M, N, seed=4)
    w3t = torch.empty(query('tvae_dense_x6_bytes', K, M) // 4, device=dev())
    call('tvae_dense_split2h', W.to(dev()), K, w3t, w3t.numel() * 4, K, M, 1, None, None)
    dX = torch.full((K, N), float('nan'), device=dev())
    dmax = (d.abs().max() * slack).reshape(1).to(dev())
    call('tvae_linear_dgrad_x6', w3t, d.to(dev()), None, None, dX, M, N, K, N, N, 0, SLOPE, parts=2, x_amax=dmax)
    assert rel_err(dX, W.double().t() @ d.double()) < GEMM_TOL['f32']
    # plain weight gradient dW = d X^T
    ws = torch.empty(query('tvae_linear_wgrad_x6_ws_floats', M, N, K), device=dev())
    dW = torch.full((M, K), float('nan'), device=dev())
    call('tvae_linear_wgrad_x6', d.to(dev()), X.to(dev()), dW, ws, ws.numel(), M, N, K, N, N, 0, vg_slope=SLOPE, parts=2,
         a_amax=dmax, x_amax=xmax)
    assert rel_err(dW, d.double() @ X.double().t()) < GEMM_TOL['f32']


def row_rel_err(got, ref, dim=0):
    """Largest PER-ROW relative error: max over the slices along `dim` of |got - ref|_2 / |ref|_2 (slices that are
    exactly zero in the reference must be exactly zero)."""
    g = got.detach().double().cpu().movedim(dim, 0).reshape(got.shape[dim], -1)
    r = ref.detach().double().cpu().movedim(dim, 0).reshape(ref.shape[dim], -1)
    num, den = (g - r).norm(dim=1), r.norm(dim=1)
    assert bool((num[den == 0] == 0).all())
    return float((num[den > 0] / den[den > 0]).max())


ROW_TOL = 1e-5          # per-ROW relative error against fp64, rows scaled by 2^-16 .. 2^-32 inside a tensor


@pytest.mark.parametrize('e', [16, 24, 32])
def test_h3_row_dynamic_range_decoder(e):
    """h3 (parts = 2) with ONE ROW of an operand 2^-e below the rest of its tensor: the output row / column that row feeds
    must be as accurate RELATIVE TO ITSELF as every other one (round 3 scaled per tensor: 4.8e-5 at e = 24, 1.3e-2 at e = 32).
    Decoder launches: forward (a row of W), two-valued data gradient (a column of W = a row of W^T), weight gradient from sign
    bits against the recomputed operand (a hidden unit of the coordinate layer = a row of the X operand)."""
    from tvae._lib import query
    s = 2.0 ** -e
    F_, B, Np, M, act = 512, 2, 256, 512, 1
    Nt = B * Np
    r0, k0, u0 = 37, 301, 100
    xr = rnd(Nt, 2, seed=1).to(dev())
    Wc, bc, LB = rnd(F_, 2, seed=2), rnd(F_, seed=3), rnd(B, F_, seed=4)
    Wc[u0] *= s; bc[u0] *= s; LB[:, u0] *= s             # hidden unit u0 of the coordinate layer: h0[u0][:] is 2^-e small
    Wc, bc, LB = Wc.to(dev()), bc.to(dev()), LB.to(dev())
    h0 = torch.empty(F_, Nt, device=dev())
    call('tvae_dec_l0_fwd', xr, Wc, bc, LB, h0, Nt, F_, Nt, Np, act, SLOPE)
    H0 = h0.double().cpu()
    W, b = rnd(M, F_, seed=5, scale=F_ ** -0.5), rnd(M, seed=6)
    W[r0] *= s; b[r0] *= s                                # output row r0 of the layer
    W[:, k0] *= s                                         # input feature k0: row k0 of W^T (the data gradient's operand)
    wo, gy = rnd(M, seed=8), rnd(Nt, seed=9)
    va = dict(va_xr=xr, va_wc=Wc, va_bc=bc, va_lb=LB, va_np=Np)
    w3 = torch.empty(query('tvae_dense_x6_bytes', M, F_) // 4, device=dev())
    call('tvae_dense_split2h', W.to(dev()), F_, w3, w3.numel() * 4, M, F_, 0, None, None)
    Y = torch.empty(M, Nt, device=dev())
    bits = torch.empty(M, Nt // 32, dtype=torch.int32, device=dev())
    call('tvae_linear_fwd_x6', w3, None, b.to(dev()), None, Y, M, Nt, F_, Nt, Nt, act, SLOPE, **va, sign_bits=bits, parts=2)
    ref_Y = act_ref(W.double() @ H0 + b.double()[:, None], act)
    assert row_rel_err(Y, ref_Y) < ROW_TOL
    assert float(ref_Y[r0].abs().max()) < 64 * s          # (the scaled row really is that small)
    Yd = Y.double().cpu()
    w3t = torch.empty(query('tvae_dense_x6_bytes', F_, M) // 4, device=dev())
    csum = torch.empty(F_, device=dev())
    call('tvae_dense_split2h', W.to(dev()), F_, w3t, w3t.numel() * 4, F_, M, 1, wo.to(dev()), csum)
    dX = torch.empty(F_, Nt, device=dev())
    rs_part = torch.empty((Nt // 128) * M * 2, device=dev())
    gys = gy.sum().reshape(1).to(dev())
    rs_db, rs_dwo = torch.empty(M, device=dev()), torch.empty(M, device=dev())
    call('tvae_linear_dgrad_x6', w3t, Y, None, h0, dX, M, Nt, F_, Nt, Nt, 1, SLOPE, vg_gy=gy.to(dev()), vg_csum=csum,
         rs_part=rs_part, rs_part_floats=rs_part.numel(), rs_wo=wo.to(dev()), rs_gysum=gys, rs_db=rs_db, rs_dwo=rs_dwo, parts=2)
    d = wo.double()[:, None] * gy.double()[None, :] * dact_ref(Yd, 1)
    ref_dX = (W.double().t() @ d) * dact_ref(H0, 1)
    assert row_rel_err(dX, ref_dX) < ROW_TOL
    ws = torch.empty(query('tvae_linear_wgrad_x6_ws_floats', M, Nt, F_), device=dev())
    dW = torch.empty(M, F_, device=dev())
    call('tvae_linear_wgrad_x6', None, None, dW, ws, ws.numel(), M, Nt, F_, Nt, Nt, 0, vg_wo=wo.to(dev()), vg_gy=gy.to(dev()),
         vg_act=1, vg_slope=SLOPE, **va, vg_bits=bits, parts=2)
    ref_dW = d @ H0.t()
    assert row_rel_err(dW, ref_dW, dim=1) < ROW_TOL      # per COLUMN of dW = per row of the X operand
    assert float(ref_dW[:, u0].abs().max()) < 1e4 * s
    # ADVICE r04 / ABI 6: the same weight gradient with its X operand read from MEMORY (Fourier decoders, stored first layers):
    # one bound per ROW of X -- (|w0| + |w1|) max |x'| + max_b |bc + lb|, times max |gy| -- keeps the small unit's column
    # exact to itself; with ONE bound for the tensor it loses the bits the unit lies below the others (measured here)
    rows = ((Wc.abs().sum(1) * xr.abs().max() + (bc[None, :] + LB).abs().amax(0)) * gy.abs().max()).contiguous()
    dWm = torch.empty(M, F_, device=dev())
    call('tvae_linear_wgrad_x6', None, h0, dWm, ws, ws.numel(), M, Nt, F_, Nt, Nt, 0, vg_wo=wo.to(dev()), vg_gy=gy.to(dev()),
         vg_act=1, vg_slope=SLOPE, vg_bits=bits, parts=2, x_amax=rows, x_amax_rows=1)
    assert row_rel_err(dWm, ref_dW, dim=1) < ROW_TOL
    if e >= 24:
        dW1 = torch.empty(M, F_, device=dev())
        call('tvae_linear_wgrad_x6', None, h0, dW1, ws, ws.numel(), M, Nt, F_, Nt, Nt, 0, vg_wo=wo.to(dev()),
             vg_gy=gy.to(dev()), vg_act=1, vg_slope=SLOPE, vg_bits=bits, parts=2, x_amax=rows.amax().reshape(1))
        err1 = float(((dW1.double().cpu() - ref_dW)[:, u0]).abs().max() / ref_dW[:, u0].abs().max())
        assert err1 > 10 * ROW_TOL, err1                  # (the per-tensor bound really is the weaker form: the reason for the rows)


@pytest.mark.parametrize('e', [16, 24, 32])
@pytest.mark.parametrize('B,n,k,pad,C,R', [(24, 64, 64, 16, 16, 8), (6, 28, 28, 8, 16, 8), (2, 96, 32, 16, 4, 4)])
def test_h3_row_dynamic_range_conv1(B, n, k, pad, C, R, e):
    """The frequency-domain lifting convolution in h3 with one FILTER (all its spectrum rows) and one IMAGE 2^-e below the
    rest: the outputs of that filter / that image, and that filter's weight gradient, to 1e-5 relative to themselves (ring,
    register-staged and generic transforms along w)."""
    from tvae._lib import query
    s = 2.0 ** -e
    Cin = 1
    c0, b0 = 3, 1
    y = torch.rand(B, Cin, n, n, generator=torch.Generator().manual_seed(1))
    y[b0] *= s
    bank = rnd(C * R, Cin * k * k, seed=2, scale=(Cin * k * k) ** -0.5)
    bank.view(C, R, -1)[c0] *= s
    Ho = n + 2 * pad - k + 1
    ref = F.conv2d(y.double(), bank.double().view(C * R, Cin, k, k), None, 1, pad).view(B, C, R, Ho, Ho)
    at = torch.zeros(query('tvae_conv1_dft_at_floats', B, Cin, n, k, pad, C, R), device=dev())
    ws = torch.empty(query('tvae_conv1_dft_ws_floats', B, Cin, n, k, pad, C, R), device=dev())
    out = torch.empty(C, B * R * Ho * Ho, device=dev())
    call('tvae_conv1_fwd_dft', y.to(dev()), bank.to(dev()), None, out, at, ws, ws.numel(), B, Cin, n, k, pad, C, R, 0, SLOPE, 2)
    got = out.view(C, B, R, Ho, Ho).permute(1, 0, 2, 3, 4)
    # per (image, filter) block: the dim image under the dim filter is 2^-2e below the rest
    g2 = got.reshape(B * C, -1)
    r2 = ref.reshape(B * C, -1)
    assert row_rel_err(g2, r2) < ROW_TOL
    # the per-channel maxima the output transform leaves for the encoder tail (last C floats behind A^T)
    assert torch.allclose(at[-C:].cpu(), got.abs().amax(dim=(0, 2, 3, 4)).cpu(), rtol=0, atol=0)
    g = rnd(B, C, R, Ho, Ho, seed=4)
    g[:, c0] *= s                                         # the gradient that reaches a dead filter
    ref_g = torch.nn.grad.conv2d_weight(y.double(), (C * R, Cin, k, k), g.double().view(B, C * R, Ho, Ho), padding=pad)
    dpre = g.permute(1, 0, 2, 3, 4).contiguous().view(C, -1).to(dev())
    dbank = torch.empty(C * R, Cin * k * k, device=dev())
    call('tvae_conv1_wgrad_dft', dpre, at, dbank, None, ws, ws.numel(), B, Cin, n, k, pad, C, R, 2)
    assert row_rel_err(dbank.view(C * R, -1), ref_g.reshape(C * R, -1)) < ROW_TOL


@pytest.mark.parametrize('e', [16, 24, 32])
def test_h3_row_dynamic_range_enc_tail(e):
    """The fused encoder tail in h3 with rows of its operands 2^-e below the rest: a row of W2 (forward), a column of W2
    (data gradient), a channel of A1 and a column of Wh (= a row of dH) in the weight gradient."""
    from tvae._lib import query
    from tvae.ops import _enc_tail_perm
    s = 2.0 ** -e
    C, nh, N = 128, 7, 4096
    r0, k0, a0, h0_ = 5, 77, 40, 19
    W2, b2 = rnd(C, C, seed=1, scale=C ** -0.5), rnd(C, seed=2)
    Wh, bh = rnd(nh, C, seed=3, scale=C ** -0.5), rnd(nh, seed=4)
    A1 = rnd(C, N, seed=5)
    W2[r0] *= s; b2[r0] *= s
    W2[:, k0] *= s
    A1[a0] *= s
    Wh[:, h0_] *= s
    a1max = A1.abs().amax(dim=1).contiguous().to(dev())
    w32 = torch.empty(query('tvae_dense_x6_bytes', C, C) // 4, device=dev())
    call('tvae_dense_split2h', W2.to(dev()), C, w32, w32.numel() * 4, C, C, 0, None, None)
    H = torch.empty(C, N, device=dev())
    heads = torch.empty(nh, N, device=dev())
    bits_h = torch.zeros(N, 4, dtype=torch.int32, device=dev())
    bits_a = torch.zeros(N, 4, dtype=torch.int32, device=dev())
    call('tvae_enc_tail_fwd_x6', w32, A1.to(dev()), N, b2.to(dev()), Wh.to(dev()), bh.to(dev()), nh, H, N, heads, N, bits_h, bits_a,
         C, N, 1, SLOPE, 2, a1max)
    Hr = act_ref(W2.double() @ A1.double() + b2.double()[:, None], 1)
    assert row_rel_err(H, Hr) < ROW_TOL
    Hs = H.double().cpu()
    dheads = rnd(nh, N, seed=6)
    w3p = torch.empty(query('tvae_dense_x6_bytes', C, C) // 4, device=dev())
    call('tvae_dense_split2h', W2.t()[:, _enc_tail_perm(dev()).cpu()].contiguous().to(dev()), C, w3p, w3p.numel() * 4, C, C, 0,
         None, None)
    wh3 = torch.empty(query('tvae_dense_x6_bytes', C, nh) // 4, device=dev())
    call('tvae_dense_split3', Wh.to(dev()), C, wh3, wh3.numel() * 4, C, nh, 1, None, None)
    dA1 = torch.empty(C, N, device=dev())
    call('tvae_enc_tail_dgrad_x6', w3p, wh3, dheads.to(dev()), N, nh, bits_h, bits_a, dA1, N, C, N, SLOPE, 2)
    dH = (Wh.double().t() @ dheads.double()) * dact_ref(Hs, 1)
    ref = (W2.double().t() @ dH) * dact_ref(A1.double(), 1)
    assert row_rel_err(dA1, ref) < ROW_TOL
    wsl = torch.empty(query('tvae_enc_tail_wgrad_x6_ws_floats', N), device=dev())
    dW2 = torch.empty(C, C, device=dev())
    call('tvae_enc_tail_wgrad_x6', A1.to(dev()), N, dheads.to(dev()), N, nh, bits_h, Wh.to(dev()), dW2, wsl, wsl.numel(), C, N,
         SLOPE, 2, a1max)
    ref_w = dH @ A1.double().t()
    assert row_rel_err(dW2, ref_w, dim=0) < ROW_TOL      # rows = rows of dH (column h0_ of Wh)
    assert row_rel_err(dW2, ref_w, dim=1) < ROW_TOL      # columns = channels of A1


@pytest.mark.parametrize('F_,B,Np,act,has_lb', [(512, 3, 256, 1, True), (300, 2, 384, 2, True), (256, 2, 128, 1, False)])
def test_linear_x6_recomputed_first_layer_operand(F_, B, Np, act, has_lb):
    """The output of the coordinate layer formed inside its three consumers (forward X, data-gradient mask, weight-gradient
    X) instead of being read: bitwise the same results as with the tensor written by tvae_dec_l0_fwd."""
    from tvae._lib import query
    Nt, M = B * Np, F_
    xr, Wc, bc = rnd(Nt, 2, seed=1).to(dev()), rnd(F_, 2, seed=2).to(dev()), rnd(F_, seed=3).to(dev())
    LB = rnd(B, F_, seed=4).to(dev()) if has_lb else None
    h0 = torch.empty(F_, Nt, device=dev())
    call('tvae_dec_l0_fwd', xr, Wc, bc, LB, h0, Nt, F_, Nt, Np, act, SLOPE)
    pre = (Wc.double().cpu() @ xr.double().cpu().t() + bc.double().cpu()[:, None] +
           (LB.double().cpu().t().repeat_interleave(Np, dim=1) if has_lb else 0.0))
    assert rel_err(h0, act_ref(pre, act)) < TOL
    W, b, d = rnd(M, F_, seed=5, scale=F_ ** -0.5), rnd(M, seed=6), rnd(M, Nt, seed=7).to(dev())
    w3 = torch.empty(query('tvae_dense_x6_bytes', M, F_) // 4, device=dev())
    w3t = torch.empty(query('tvae_dense_x6_bytes', F_, M) // 4, device=dev())
    call('tvae_dense_split3', W.to(dev()), F_, w3, w3.numel() * 4, M, F_, 0, None, None)
    call('tvae_dense_split3', W.to(dev()), F_, w3t, w3t.numel() * 4, F_, M, 1, None, None)
    va = dict(va_xr=xr, va_wc=Wc, va_bc=bc, va_lb=LB, va_np=Np)
    # forward
    Y = [torch.empty(M, Nt, device=dev()) for _ in range(2)]
    call('tvae_linear_fwd_x6', w3, h0, b.to(dev()), None, Y[0], M, Nt, F_, Nt, Nt, act, SLOPE, parts=3)
    call('tvae_linear_fwd_x6', w3, None, b.to(dev()), None, Y[1], M, Nt, F_, Nt, Nt, act, SLOPE, **va, parts=3)
    assert torch.equal(Y[0], Y[1])
    assert rel_err(Y[0], act_ref(W.double() @ h0.double().cpu() + b.double()[:, None], act)) < GEMM_TOL['f32']
    # data gradient with the fused coordinate-layer backward
    outs = []
    for virt in (False, True):
        gxr = torch.empty(Nt, 2, device=dev())
        part = torch.empty((Nt // 128) * F_ * 3, device=dev())
        call('tvae_linear_dgrad_x6', w3t, d, None, None if virt else h0, None, M, Nt, F_, Nt, Nt, act, SLOPE, in_xr=xr,
             in_wc=Wc, in_gxr=gxr, in_part=part, in_part_floats=part.numel(), in_bc=bc if virt else None,
             in_lb=LB if virt else None, in_np=Np if virt else 0, parts=3)
        outs.append((gxr, part))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    d0 = (W.double().t() @ d.double().cpu()) * dact_ref(h0.double().cpu(), act)
    assert rel_err(outs[1][0], d0.t() @ Wc.double().cpu()) < GEMM_TOL['f32']
    # weight gradient
    ws = torch.empty(1 << 26, device=dev())       # >= tvae_linear_wgrad_x6_ws_floats(M, N, K): slices x M x K
    dW = [torch.empty(M, F_, device=dev()) for _ in range(2)]
    call('tvae_linear_wgrad_x6', d, h0, dW[0], ws, ws.numel(), M, Nt, F_, Nt, Nt, 0, vg_act=act, vg_slope=SLOPE, parts=3)
    call('tvae_linear_wgrad_x6', d, None, dW[1], ws, ws.numel(), M, Nt, F_, Nt, Nt, 0, vg_act=act, vg_slope=SLOPE, **va,
         parts=3)
    assert torch.equal(dW[0], dW[1])
    assert rel_err(dW[1], d.double().cpu() @ h0.double().cpu().t()) < GEMM_TOL['f32']
    # images that are not whole column tiles are refused
    with pytest.raises(Exception):
        call('tvae_linear_fwd_x6', w3, None, b.to(dev()), None, Y[1], M, Nt, F_, Nt, Nt, act, SLOPE, va_xr=xr, va_wc=Wc,
             va_bc=bc, va_lb=LB, va_np=96, parts=3)


def test_linear_fwd_x6_h3_refuses_before_its_bound_prepass():
    """h3 forward with the recomputed first-layer operand (parts = 2, va_*): the entry point forms the operand's bound words in
    the trailer of the cell buffer (behind the row maxima of tvae_dense_split2h) before its GEMM.  With va_np = 96 (images that
    are not whole column tiles) the call is refused, and refused BEFORE that pre-pass: the NaN-filled output stays all NaN and
    the whole cell buffer is bit for bit what it was.  The refused call comes first, while the bound words still hold the zeros
    the buffer was made with (a pre-pass that ran would leave the bounds there; after a valid call it would only rewrite the
    same values).  With va_np = 128 the same call is valid: fp64 reference at the fp32 tolerance."""
    M, K, N, Np, act = 32, 64, 384, 128, 1
    xr, Wc, bc, LB = rnd(N, 2, seed=1), rnd(K, 2, seed=2), rnd(K, seed=3), rnd(N // Np, K, seed=4)
    W, b = rnd(M, K, seed=5, scale=K ** -0.5), rnd(M, seed=6)
    w3 = torch.zeros(query('tvae_dense_x6_bytes', M, K) // 4, device=dev())
    call('tvae_dense_split2h', W.to(dev()), K, w3, w3.numel() * 4, M, K, 0, None, None)
    va = dict(va_xr=xr.to(dev()), va_wc=Wc.to(dev()), va_bc=bc.to(dev()), va_lb=LB.to(dev()))
    Y = torch.full((M, N), float('nan'), device=dev())
    before = w3.clone()
    with pytest.raises(Exception):
        call('tvae_linear_fwd_x6', w3, None, b.to(dev()), None, Y, M, N, K, N, N, act, SLOPE, **va, va_np=96, parts=2)
    assert bool(torch.isnan(Y).all())
    assert torch.equal(w3.view(torch.int32), before.view(torch.int32))
    call('tvae_linear_fwd_x6', w3, None, b.to(dev()), None, Y, M, N, K, N, N, act, SLOPE, **va, va_np=Np, parts=2)
    h0 = act_ref(Wc.double() @ xr.double().t() + bc.double()[:, None] + LB.double().t().repeat_interleave(Np, dim=1), act)
    assert bool(torch.isfinite(Y).all())
    assert rel_err(Y, act_ref(W.double() @ h0 + b.double()[:, None], act)) < GEMM_TOL['f32']
    assert not torch.equal(w3.view(torch.int32), before.view(torch.int32))      # (the valid call did write its bound words)


def test_reductions():
    M, N = 37, 10007
    X = rnd(M, N, seed=1)
    V = rnd(N, 3, seed=2)
    sl = 1000
    nseg = (N + sl - 1) // sl
    out = torch.empty(nseg, M, 3, device=dev())
    call('tvae_rowdot_seg', X.to(dev()), N, V.to(dev()), 3, M, N, sl, out)
    ref = torch.stack([X[:, s * sl:(s + 1) * sl].double() @ V[s * sl:(s + 1) * sl].double() for s in range(nseg)])
    assert rel_err(out, ref) < TOL
    out1 = torch.empty(nseg, M, device=dev())
    call('tvae_rowdot_seg', X.to(dev()), N, None, 1, M, N, sl, out1)
    ref1 = torch.stack([X[:, s * sl:(s + 1) * sl].double().sum(1) for s in range(nseg)])
    assert rel_err(out1, ref1) < TOL
    tot = torch.full((M,), 2.0, device=dev())
    call('tvae_seg_sum', out1, nseg, M, tot, 0.5, 1)
    assert rel_err(tot, 2.0 + 0.5 * X.double().sum(1)) < TOL


@pytest.mark.parametrize('N,rows_d,ldpad', [(32 * 700, 103, 0), (32 * 3, 128, 0), (32 * 1031, 8, 64), (32, 1, 0)])
def test_enc_tail_wgrad_wide(N, rows_d, ldpad):
    """Round 6: dW[r][c] = sum_n D[r][n] A[c][n] for two stored operands (the encoder tail's weight gradients with many head rows:
    autograd of the 1x1x1 convolutions, reference src/models.py:347-358,390-392) against float64 -- fewer chunks than
    workgroups, one chunk, padded leading dimensions, rows of both operands 2^-20 below the rest (per-row relative error of dW's
    rows AND columns), loose bounds (8x the true maxima), repeatable bit for bit."""
    from tvae._lib import query
    C = 128
    s = 2.0 ** -20
    D, A = rnd(rows_d, N, seed=1), rnd(C, N, seed=2)
    A[7] *= s
    if rows_d > 2:
        D[1] *= 2.0 ** -10
    ld = N + ldpad
    Dp = torch.full((rows_d, ld), float('nan')); Dp[:, :N] = D
    Ap = torch.full((C, ld), float('nan')); Ap[:, :N] = A
    if ldpad:
        Dp[:, N:] = 1e30; Ap[:, N:] = 1e30               # (never read)
    amax_d = (8.0 * D.abs().max()).reshape(1).to(dev())
    amax_a = (8.0 * A.abs().amax(dim=1)).contiguous().to(dev())
    ws = torch.empty(query('tvae_enc_tail_wgrad_x6_ws_floats', N), device=dev())
    out = [torch.full((C, C), float('nan'), device=dev()) for _ in range(2)]
    for o in out:
        call('tvae_enc_tail_wgrad_wide', Dp.to(dev()), ld, rows_d, Ap.to(dev()), ld, o, ws, ws.numel(), C, N, amax_d, amax_a)
    assert torch.equal(out[0][:rows_d], out[1][:rows_d])
    ref = D.double() @ A.double().t()
    got = out[0][:rows_d].double().cpu()
    assert torch.isfinite(got).all()
    assert row_rel_err(got, ref) < ROW_TOL
    assert row_rel_err(got.t(), ref.t()) < ROW_TOL
    # argument checks: ragged N, too many rows, missing bounds
    for bad in ((N + 1, rows_d, amax_d), (N, 129, amax_d), (N, rows_d, None)):
        with pytest.raises(Exception):
            call('tvae_enc_tail_wgrad_wide', Dp.to(dev()), ld, bad[1], Ap.to(dev()), ld, out[0], ws, ws.numel(), C, bad[0], bad[2], amax_a)


def test_enc_tail_wgrad_wide_galaxy_size():
    """The same entry point at the galaxy configuration's column count (8 images x 16 rotations x 129^2 positions, 103 head
    rows; BASELINE.json configs[4]) against a float64 product formed on the GPU, bounds as the product path forms them
    (max |D| measured; per-row analytic bounds of A loose by the row-sum factor)."""
    from tvae._lib import query
    C, rows_d, N = 128, 103, 8 * 16 * 129 * 129
    g = torch.Generator(device=dev()).manual_seed(3)
    D = torch.randn(rows_d, N, device=dev(), generator=g) * torch.logspace(-6, 0, rows_d, device=dev())[:, None]
    A = torch.nn.functional.leaky_relu(torch.randn(C, N, device=dev(), generator=g), SLOPE)
    amax_d = D.abs().max().reshape(1)
    amax_a = (11.0 * A.abs().amax(dim=1)).contiguous()
    ws = torch.empty(query('tvae_enc_tail_wgrad_x6_ws_floats', N), device=dev())
    out = torch.full((C, C), float('nan'), device=dev())
    call('tvae_enc_tail_wgrad_wide', D, N, rows_d, A, N, out, ws, ws.numel(), C, N, amax_d, amax_a)
    ref = D.double() @ A.double().t()
    assert row_rel_err(out[:rows_d], ref) < ROW_TOL
    assert rel_err(out[:rows_d], ref) < 1e-5        # (fp32 accumulation over 8 320 columns per workgroup: ~2e-6 measured)


@pytest.mark.parametrize('S,L', [(256, 512), (100, 130), (67, 65), (64, 7), (5, 300), (256, 3)])
def test_seg_sum_instances(S, L):
    """tvae_seg_sum picks one of three kernels by shape (one thread per output / one wave per output / 64 outputs x 16 segment
    lanes): all agree with the fp64 sum, with scaling and accumulation, and repeat bit for bit."""
    X = rnd(S, L, seed=S + L).to(dev())
    out = torch.full((L,), 3.0, device=dev())
    call('tvae_seg_sum', X, S, L, out, 0.25, 1)
    assert rel_err(out, 3.0 + 0.25 * X.double().sum(0)) < TOL
    o1, o2 = torch.empty(L, device=dev()), torch.empty(L, device=dev())
    call('tvae_seg_sum', X, S, L, o1, 1.0, 0)
    call('tvae_seg_sum', X, S, L, o2, 1.0, 0)
    assert torch.equal(o1, o2) and rel_err(o1, X.double().sum(0)) < TOL


@pytest.mark.parametrize('no', [1, 2, 3])
def test_coldot_outer_mask(no):
    M, N = 64, 1500
    X, W, b = rnd(M, N, seed=1), rnd(no, M, seed=2), rnd(no, seed=3)
    out = torch.empty(N, no, device=dev())
    call('tvae_coldot', X.to(dev()), N, M, N, W.to(dev()), 1, M, b.to(dev()), no, out)
    assert rel_err(out, (W.double() @ X.double()).t() + b.double()) < TOL
    dy = rnd(N, no, seed=4)
    D = torch.empty(M, N, device=dev())
    call('tvae_outer_mask', dy.to(dev()), no, W.to(dev()), 1, M, X.to(dev()), N, D, N, M, N, 1, SLOPE)
    ref = (W.double().t() @ dy.double().t()) * dact_ref(X.double(), 1)
    assert rel_err(D, ref) < TOL
    pre = torch.empty(M, N, device=dev())
    call('tvae_act_bwd', D, X.to(dev()), pre, M * N, 1, SLOPE)
    assert rel_err(pre, ref * dact_ref(X.double(), 1)) < TOL


@pytest.mark.parametrize('F_,N,no,act', [(64, 3000, 1, 1), (37, 2051, 2, 1), (130, 1024, 3, 2), (16, 5000, 4, 0)])
def test_dec_out_bwd(F_, N, no, act):
    gy, Wo = rnd(N, no, seed=1), rnd(no, F_, seed=2)
    H = rnd(F_, N, seed=3).clamp(-0.9, 0.9)
    D = torch.empty(F_, N, device=dev())
    npan = (N + 1023) // 1024
    part = torch.empty(npan * F_ * (1 + no), device=dev())
    tot = torch.empty(1 + no, F_, device=dev())
    call('tvae_dec_out_bwd', gy.to(dev()), no, Wo.to(dev()), H.to(dev()), N, D, N, F_, N, act, SLOPE, part,
         part.numel(), tot)
    ref = (Wo.double().t() @ gy.double().t()) * dact_ref(H.double(), act)
    assert rel_err(D, ref) < TOL
    assert rel_err(tot[0], ref.sum(1)) < TOL
    assert rel_err(tot[1:], (H.double() @ gy.double()).t()) < TOL
    small = torch.empty(4, device=dev())
    with pytest.raises(Exception):
        call('tvae_dec_out_bwd', gy.to(dev()), no, Wo.to(dev()), H.to(dev()), N, D, N, F_, N, act, SLOPE, small, 4, tot)


@pytest.mark.parametrize('F_,B,Np', [(64, 3, 784), (33, 2, 1089), (128, 2, 4096), (8, 5, 2500)])
def test_dec_in_bwd(F_, B, Np):
    Nt = B * Np
    d, xr, Wc = rnd(F_, Nt, seed=1), rnd(Nt, 2, seed=2), rnd(F_, 2, seed=3)
    cpi = (Np + 1023) // 1024
    part = torch.empty(B * cpi * F_ * 3, device=dev())
    gxr = torch.empty(Nt, 2, device=dev())
    Simg = torch.empty(B, F_, device=dev())
    dbc = torch.empty(F_, device=dev())
    dWc = torch.empty(F_, 2, device=dev())
    call('tvae_dec_in_bwd', d.to(dev()), Nt, xr.to(dev()), Wc.to(dev()), F_, B, Np, gxr, Simg, dbc, dWc, part,
         part.numel())
    dd = d.double()
    assert rel_err(gxr, dd.t() @ Wc.double()) < TOL
    assert rel_err(Simg, dd.view(F_, B, Np).sum(2).t()) < TOL
    assert rel_err(dbc, dd.sum(1)) < TOL
    assert rel_err(dWc, dd @ xr.double()) < TOL


@pytest.mark.parametrize('nh,C,N,act', [(7, 128, 8712, 1), (3, 33, 1001, 1), (8, 64, 2048, 2), (1, 16, 515, 0),
                                        (5, 128, 4356, 1)])
def test_heads_fwd_bwd(nh, C, N, act):
    W, b = rnd(nh, C, seed=1, scale=C ** -0.5), rnd(nh, seed=2)
    X = rnd(C, N, seed=3).clamp(-0.9, 0.9)
    Y = torch.empty(nh, N, device=dev())
    call('tvae_heads_fwd', W.to(dev()), X.to(dev()), N, b.to(dev()), Y, N, nh, C, N)
    assert rel_err(Y, W.double() @ X.double() + b.double()[:, None]) < TOL
    dY = rnd(nh, N, seed=4)
    dX = torch.empty(C, N, device=dev())
    npan = (N + 511) // 512
    part = torch.empty(npan * C * (nh + 1), device=dev())
    tot = torch.empty(nh + 1, C, device=dev())
    call('tvae_heads_bwd', W.to(dev()), dY.to(dev()), N, X.to(dev()), N, dX, N, nh, C, N, act, SLOPE, part,
         part.numel(), tot)
    ref = (W.double().t() @ dY.double()) * dact_ref(X.double(), act)
    assert rel_err(dX, ref) < TOL
    assert rel_err(tot[:nh], dY.double() @ X.double().t()) < TOL
    assert rel_err(tot[nh], ref.sum(1)) < TOL
    with pytest.raises(Exception):
        call('tvae_heads_fwd', W.to(dev()), X.to(dev()), N, b.to(dev()), Y, N, 9, C, N)


def _split_w(W, rows, K, transpose):
    a3 = torch.empty(query('tvae_dense_x6_bytes', rows, K) // 4, device=dev())
    call('tvae_dense_split3', W.contiguous(), W.shape[1], a3, a3.numel() * 4, rows, K, transpose, None, None)
    return a3


def _enc_tail_perm():
    from tvae.ops import _enc_tail_perm as f
    return f(dev())


@pytest.mark.parametrize('N,nh,act,parts', [(64 * 40, 7, 1, 3), (64 * 2048 + 37, 7, 1, 3), (1000, 5, 2, 3), (31, 1, 0, 3),
                                            (64 * 300, 7, 1, 1), (64 * 1024 + 36, 3, 1, 3), (4, 7, 1, 3), (32 * 9001, 7, 1, 3),
                                            (32, 2, 1, 3)])
def test_enc_tail_x6(N, nh, act, parts):
    """Fused conv2 + head projection (reference models.py:356-358, 390-392) and its fused data gradient against fp64."""
    C = 128
    W2, b2 = rnd(C, C, seed=1, scale=C ** -0.5), rnd(C, seed=2)
    Wh, bh = rnd(nh, C, seed=3, scale=C ** -0.5), rnd(nh, seed=4)
    A1 = rnd(C, N, seed=5)
    H = torch.full((C, N), float('nan'), device=dev())
    heads = torch.full((nh, N), float('nan'), device=dev())
    w3 = _split_w(W2.to(dev()), C, C, 0)
    lrelu = act == 1
    bits_h = torch.zeros(N, 4, dtype=torch.int32, device=dev()) if lrelu else None
    bits_a = torch.zeros(N, 4, dtype=torch.int32, device=dev()) if lrelu else None
    call('tvae_enc_tail_fwd_x6', w3, A1.to(dev()), N, b2.to(dev()), Wh.to(dev()), bh.to(dev()), nh, H, N, heads, N, bits_h,
         bits_a, C, N, act, SLOPE, parts)
    Hr = act_ref(W2.double() @ A1.double() + b2.double()[:, None], act)
    hr = Wh.double() @ Hr + bh.double()[:, None]
    tol = TOL if parts == 3 else 2e-2
    assert rel_err(H, Hr) < tol
    assert rel_err(heads, hr) < tol
    if parts == 3:
        # the same launch in the h3 arithmetic: two fp16 parts under the scale of max |A1| (per-channel device words from A1's producer),
        # for activations of size 1, 1e-5 and 1e3 (a bound 64 x too large must not matter either)
        w32 = torch.empty(query('tvae_dense_x6_bytes', C, C) // 4, device=dev())
        call('tvae_dense_split2h', W2.to(dev()), C, w32, w32.numel() * 4, C, C, 0, None, None)
        # (tanh at 1e3 saturates: every arithmetic then differs where a pre-activation of size 1 is a difference of terms of size 1e3)
        for sc, slack in ((1.0, 1.0), (1e-5, 1.0)) + (((1e3, 64.0),) if act != 2 else ()):
            A1s = (A1 * sc).to(dev())
            amax = (A1s.abs().amax(dim=1) * slack).contiguous()      # one maximum per channel (ABI 5), from A1's producer
            H2, h2 = torch.full((C, N), float('nan'), device=dev()), torch.full((nh, N), float('nan'), device=dev())
            call('tvae_enc_tail_fwd_x6', w32, A1s, N, b2.to(dev()), Wh.to(dev()), bh.to(dev()), nh, H2, N, h2, N, None, None, C, N,
                 act, SLOPE, 2, amax)
            Hr2 = act_ref(W2.double() @ (A1.double() * sc) + b2.double()[:, None], act)
            assert rel_err(H2, Hr2) < TOL and rel_err(h2, Wh.double() @ Hr2 + bh.double()[:, None]) < TOL, sc
        with pytest.raises(Exception):                   # h3 without the operand maximum
            call('tvae_enc_tail_fwd_x6', w32, A1.to(dev()), N, b2.to(dev()), Wh.to(dev()), bh.to(dev()), nh, H, N, heads, N, None,
                 None, C, N, act, SLOPE, 2, None)
    with pytest.raises(Exception):                       # only the 128-channel layer is built
        call('tvae_enc_tail_fwd_x6', w3, A1.to(dev()), N, b2.to(dev()), Wh.to(dev()), bh.to(dev()), nh, H, N, heads, N, None,
             None, 64, N, act, SLOPE, parts)
    if not lrelu:
        with pytest.raises(Exception):                   # the sign words describe a LeakyReLU
            junk = torch.zeros(N, 4, dtype=torch.int32, device=dev())
            call('tvae_enc_tail_fwd_x6', w3, A1.to(dev()), N, b2.to(dev()), Wh.to(dev()), bh.to(dev()), nh, H, N, heads, N,
                 junk, junk, C, N, act, SLOPE, parts)
        return
    # sign words: bit (r & 31) of word r >> 5 of column n
    def unpack(b):
        w = b.cpu().numpy().astype(np.uint32)                              # [N][4]
        return torch.from_numpy(((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(N, 128).T.copy()).bool()
    assert torch.equal(unpack(bits_a), A1 > 0)
    assert torch.equal(unpack(bits_h), H.cpu() > 0)
    dheads = rnd(nh, N, seed=6)
    w3p = _split_w(W2.t()[:, _enc_tail_perm().cpu()].contiguous().to(dev()), C, C, 0)
    wh3 = torch.empty(query('tvae_dense_x6_bytes', C, nh) // 4, device=dev())
    call('tvae_dense_split3', Wh.to(dev()), C, wh3, wh3.numel() * 4, C, nh, 1, None, None)
    dA1 = torch.full((C, N), float('nan'), device=dev())
    call('tvae_enc_tail_dgrad_x6', w3p, wh3, dheads.to(dev()), N, nh, bits_h, bits_a, dA1, N, C, N, SLOPE, parts)
    Hs = H.cpu().double()                                # the mask of the kernel's own forward (kinks of fp64 H may differ)
    dH = (Wh.double().t() @ dheads.double()) * dact_ref(Hs, 1)
    ref = (W2.double().t() @ dH) * dact_ref(A1.double(), 1)
    assert rel_err(dA1, ref) < tol
    if parts == 3:
        # the same launch in the h3 arithmetic (parts = 2: the 128 x 128 GEMM on two fp16 parts with the exact scale of each
        # 32-column chunk; the skinny head-row GEMM stays in the three-part split), also for gradients of size 1e-7
        w3p2 = torch.empty(query('tvae_dense_x6_bytes', C, C) // 4, device=dev())
        call('tvae_dense_split2h', W2.t()[:, _enc_tail_perm().cpu()].contiguous().to(dev()), C, w3p2, w3p2.numel() * 4, C, C, 0,
             None, None)
        for sc in (1.0, 1e-7):
            dA2 = torch.full((C, N), float('nan'), device=dev())
            call('tvae_enc_tail_dgrad_x6', w3p2, wh3, (dheads * sc).to(dev()), N, nh, bits_h, bits_a, dA2, N, C, N, SLOPE, 2)
            assert rel_err(dA2, ref * sc) < TOL, sc
    # conv2's weight gradient in one pass (dH formed from the head gradients and the sign words, never stored), and the
    # sums-only form of tvae_heads_bwd (dX = NULL) that supplies dWh / db2 beside it
    if N % 32 == 0:
        wsl = torch.full((query('tvae_enc_tail_wgrad_x6_ws_floats', N),), float('nan'), device=dev())
        dW2 = torch.full((C, C), float('nan'), device=dev())
        call('tvae_enc_tail_wgrad_x6', A1.to(dev()), N, dheads.to(dev()), N, nh, bits_h, Wh.to(dev()), dW2, wsl, wsl.numel(), C, N,
             SLOPE, parts)
        assert rel_err(dW2, dH @ A1.double().t()) < tol
        if parts == 3:                       # the same in the h3 arithmetic, also for head gradients of size 1e-7
            for sc in (1.0, 1e-7):
                dW2h = torch.full((C, C), float('nan'), device=dev())
                call('tvae_enc_tail_wgrad_x6', A1.to(dev()), N, (dheads * sc).to(dev()), N, nh, bits_h, Wh.to(dev()), dW2h, wsl,
                     wsl.numel(), C, N, SLOPE, 2, A1.abs().amax(dim=1).contiguous().to(dev()))
                assert rel_err(dW2h, (dH @ A1.double().t()) * sc) < TOL, sc
        npan = (N + 511) // 512
        part = torch.empty(npan * C * (nh + 1), device=dev())
        tot = torch.empty(nh + 1, C, device=dev())
        call('tvae_heads_bwd', Wh.to(dev()), dheads.to(dev()), N, H, N, None, N, nh, C, N, 1, SLOPE, part, part.numel(), tot)
        assert rel_err(tot[:nh], dheads.double() @ Hs.t()) < TOL and rel_err(tot[nh], dH.sum(1)) < 1e-4
    else:
        with pytest.raises(Exception):                   # whole 32-column chunks only (the unfused path takes the rest)
            call('tvae_enc_tail_wgrad_x6', A1.to(dev()), N, dheads.to(dev()), N, nh, bits_h, Wh.to(dev()), dA1, dA1, dA1.numel(),
                 C, N, SLOPE, parts)


def test_enc_tail_x6_full_size_properties():
    """The fused encoder tail at the benchmark's full size (N = 256 * 8 * 33 * 33 columns): two runs are bitwise
    identical (persistent workgroups, no atomics), a random sample of columns matches fp64, and every sign word equals
    the sign of what was stored."""
    C, nh, N = 128, 7, 256 * 8 * 33 * 33
    g = torch.Generator(device=dev()).manual_seed(11)
    W2 = torch.randn(C, C, device=dev(), generator=g) * C ** -0.5
    b2 = torch.randn(C, device=dev(), generator=g)
    Wh = torch.randn(nh, C, device=dev(), generator=g) * C ** -0.5
    bh = torch.randn(nh, device=dev(), generator=g)
    A1 = torch.randn(C, N, device=dev(), generator=g)
    dheads = torch.randn(nh, N, device=dev(), generator=g)
    w3 = _split_w(W2, C, C, 0)
    w3p = _split_w(W2.t()[:, _enc_tail_perm()].contiguous(), C, C, 0)
    wh3 = torch.empty(query('tvae_dense_x6_bytes', C, nh) // 4, device=dev())
    call('tvae_dense_split3', Wh, C, wh3, wh3.numel() * 4, C, nh, 1, None, None)
    outs = []
    for _ in range(2):
        H = torch.empty(C, N, device=dev())
        heads = torch.empty(nh, N, device=dev())
        bits = torch.zeros(2, N, 4, dtype=torch.int32, device=dev())
        dA1 = torch.empty(C, N, device=dev())
        call('tvae_enc_tail_fwd_x6', w3, A1, N, b2, Wh, bh, nh, H, N, heads, N, bits[0], bits[1], C, N, 1, SLOPE, 3)
        call('tvae_enc_tail_dgrad_x6', w3p, wh3, dheads, N, nh, bits[0], bits[1], dA1, N, C, N, SLOPE, 3)
        outs.append((H, heads, bits, dA1))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    H, heads, bits, dA1 = outs[0]
    cols = torch.randint(0, N, (4096,), device=dev(), generator=g)
    cols[:64] = torch.arange(N - 64, N, device=dev())                      # the last chunks too
    Hr = act_ref(W2.double() @ A1[:, cols].double() + b2.double()[:, None], 1)
    assert rel_err(H[:, cols], Hr) < TOL
    assert rel_err(heads[:, cols], Wh.double() @ Hr + bh.double()[:, None]) < TOL
    dH = (Wh.double().t() @ dheads[:, cols].double()) * dact_ref(H[:, cols].double(), 1)
    assert rel_err(dA1[:, cols], (W2.double().t() @ dH) * dact_ref(A1[:, cols].double(), 1)) < TOL
    shifts = torch.arange(32, device=dev(), dtype=torch.int32)
    for t, w in ((H, bits[0]), (A1, bits[1])):
        got = ((w[cols][:, :, None] >> shifts) & 1).reshape(-1, 128).t().bool()
        assert torch.equal(got, t[:, cols] > 0)
    # the weight gradients of the same step at full size (every CU busy): dH, dWh, db2 from tvae_heads_bwd, dW2 from the
    # fp32-MFMA reduction over all 2.2 M columns, against fp64 sums
    dH = torch.empty(C, N, device=dev())
    npan = (N + 511) // 512
    part = torch.empty(npan * C * (nh + 1), device=dev())
    tot = torch.empty(nh + 1, C, device=dev())
    call('tvae_heads_bwd', Wh, dheads, N, H, N, dH, N, nh, C, N, 1, SLOPE, part, part.numel(), tot)
    dW2 = torch.empty(C, C, device=dev())
    ws = torch.empty(1 << 24, device=dev())
    call('tvae_linear_wgrad', dH, A1, dW2, ws, ws.numel(), C, N, C, N, N, 0)
    dHr = torch.zeros(C, C, dtype=torch.float64, device=dev())
    dWhr = torch.zeros(nh, C, dtype=torch.float64, device=dev())
    dbr = torch.zeros(C, dtype=torch.float64, device=dev())
    step = 1 << 18                                       # fp64 references in column slices (memory)
    for c0 in range(0, N, step):
        sl = slice(c0, min(N, c0 + step))
        Hd = H[:, sl].double()
        dHd = (Wh.double().t() @ dheads[:, sl].double()) * dact_ref(Hd, 1)
        dHr += dHd @ A1[:, sl].double().t()
        dWhr += dheads[:, sl].double() @ Hd.t()
        dbr += dHd.sum(1)
    assert rel_err(tot[:nh], dWhr) < TOL
    assert rel_err(tot[nh], dbr) < 1e-4
    assert rel_err(dW2, dHr) < TOL
    # the one-pass form (dH never stored): same sums, bitwise repeatable
    wsl = torch.empty(query('tvae_enc_tail_wgrad_x6_ws_floats', N), device=dev())
    dW2f, dW2g = torch.empty(C, C, device=dev()), torch.empty(C, C, device=dev())
    call('tvae_enc_tail_wgrad_x6', A1, N, dheads, N, nh, bits[0], Wh, dW2f, wsl, wsl.numel(), C, N, SLOPE, 3)
    call('tvae_enc_tail_wgrad_x6', A1, N, dheads, N, nh, bits[0], Wh, dW2g, wsl, wsl.numel(), C, N, SLOPE, 3)
    assert torch.equal(dW2f, dW2g) and rel_err(dW2f, dHr) < TOL
    tot2 = torch.empty(nh + 1, C, device=dev())
    call('tvae_heads_bwd', Wh, dheads, N, H, N, None, N, nh, C, N, 1, SLOPE, part, part.numel(), tot2)
    assert torch.equal(tot2, tot)


@pytest.mark.parametrize('C,B,R,Ho,act', [(8, 3, 4, 9, 1), (128, 5, 8, 29, 1), (16, 2, 16, 7, 2), (5, 1, 8, 3, 0)])
def test_rot_pool(C, B, R, Ho, act):
    """fc_r pooling over the rotation axis (reference models.py:303-305) and its backward through the activation."""
    P = Ho * Ho
    A1 = rnd(C, B, R, P, seed=1).clamp(-0.9, 0.9)
    fw, fb = rnd(R, seed=2), rnd(1, seed=3)
    X = torch.empty(C, B * P, device=dev())
    call('tvae_rot_pool_fwd', A1.to(dev()), fw.to(dev()), fb.to(dev()), X, C, B, R, P)
    ref = torch.einsum('cbrp,r->cbp', A1.double(), fw.double()) + fb.double()
    assert rel_err(X.view(C, B, P), ref) < TOL
    dX = rnd(C, B, P, seed=4)
    dA1 = torch.empty(C, B, R, P, device=dev())
    nb = min(1024, (C * B * P + 255) // 256)
    part = torch.empty(nb * (R + 1), device=dev())
    dtot = torch.empty(R + 1, device=dev())
    call('tvae_rot_pool_bwd', A1.to(dev()), dX.to(dev()), fw.to(dev()), dA1, part, part.numel(), dtot, C, B, R, P, act,
         SLOPE)
    dref = dX.double()[:, :, None, :] * fw.double()[None, None, :, None] * dact_ref(A1.double(), act)
    assert rel_err(dA1, dref) < TOL
    assert rel_err(dtot[:R], torch.einsum('cbrp,cbp->r', A1.double(), dX.double())) < TOL
    assert rel_err(dtot[R], dX.double().sum()) < 1e-4
    with pytest.raises(Exception):                       # short partial-sum workspace
        call('tvae_rot_pool_bwd', A1.to(dev()), dX.to(dev()), fw.to(dev()), dA1, part, R, dtot, C, B, R, P, act, SLOPE)


def test_coord():
    B, n = 3, 9
    xc = O.image_coords(n)
    dx = rnd(B, 2, seed=1, scale=0.2).requires_grad_(True)
    th = rnd(B, seed=2).requires_grad_(True)
    x = xc.expand(B, -1, -1) - dx.unsqueeze(1)
    rot = torch.stack([torch.stack([torch.cos(th), torch.sin(th)], 1),
                       torch.stack([-torch.sin(th), torch.cos(th)], 1)], 1)
    ref = torch.bmm(x, rot)
    g = rnd(B, n * n, 2, seed=3)
    (ref * g).sum().backward()
    from tvae import ops
    dxg = dx.detach().to(dev()).requires_grad_(True)
    thg = th.detach().to(dev()).requires_grad_(True)
    xr = ops.CoordFn.apply(xc.to(dev()), dxg, thg)
    assert rel_err(xr, ref) < 1e-6
    (xr * g.to(dev())).sum().backward()
    assert rel_err(dxg.grad, dx.grad) < TOL and rel_err(thg.grad, th.grad) < TOL


@pytest.mark.parametrize('kind,name,B,L,spikes', [
    pytest.param(k_, n_, B_, L_, s_, id=f'{k_}-{n_}' + i_)
    for B_, L_, s_, i_ in ((3, 500, False, ''), (3, 500, True, '-spikes'), (2, 16384 + 37, True, '-B2-L16421-spikes'),
                           (300, 20000, False, '-B300-L20000'))
    for k_, n_ in ((0, 'bce'), (1, 'gauss'), (2, 'gauss_var'))])
def test_loglik(kind, name, B, L, spikes):
    """Against float64.  (2, 16 384 + 37): the 1024-thread instance of the forward (B < 256 and L >= 16 384) with a ragged
    last round; (300, 20 000): the 256-thread instance just beyond that boundary in B; spikes: logits / means of +-60 in a
    few positions (exp(-|x|) underflows towards 0, the stable form of the BCE has to hold)."""
    y = torch.rand(B, L, generator=torch.Generator().manual_seed(1)).double()
    yh = rnd(B, 2 * L if kind == 2 else L, seed=2, scale=2.0)
    if spikes:
        yh[0, 0], yh[0, L - 1], yh[B - 1, L // 2], yh[B - 1, 1] = 60.0, -60.0, 60.0, -60.0
    yh = yh.double().requires_grad_(True)
    w = rnd(B, seed=3).double()
    if kind == 0:
        per = -(F.binary_cross_entropy_with_logits(yh, y, reduction='none')).sum(1)
    elif kind == 1:
        per = -0.5 * ((yh - y) ** 2).sum(1)
    else:
        per = -0.5 * ((yh[:, :L] - y) ** 2 / torch.exp(yh[:, L:]) + yh[:, L:]).sum(1)
    (per * w).sum().backward()
    assert abs(float(per.mean()) - float(O.likelihood_logp(yh.detach(), y, name))) < 1e-3 * abs(float(per.mean()))
    from tvae import ops
    yg = yh.detach().float().to(dev()).requires_grad_(True)
    lp = ops.LogLikFn.apply(yg, y.float().to(dev()), kind)
    assert rel_err(lp, per) < TOL
    (lp * w.float().to(dev())).sum().backward()
    assert rel_err(yg.grad, yh.grad) < TOL


def test_adam_flat():
    """n > 2048 x 256: the grid-stride loop of the kernel takes more than one round; grad_scale (the data-parallel average)
    against torch's Adam on the scaled gradient, moments included."""
    for n, grad_scale in ((10001, 1.0), (2048 * 256 + 12345, 0.25)):
        _adam_flat_case(n, grad_scale)


def _adam_flat_case(n, grad_scale):
    p0, steps = rnd(n, seed=1), 3
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=2e-4)
    p = p0.clone().to(dev())
    m = torch.zeros(n, device=dev())
    v = torch.zeros(n, device=dev())
    from tvae import ops
    for s in range(steps):
        g = rnd(n, seed=10 + s)
        p_ref.grad = g * grad_scale                  # 0.25: exact in fp32
        opt.step()
        ops.adam_flat(p, g.to(dev()), m, v, s + 1, 2e-4, grad_scale=grad_scale)
    assert rel_err(p, p_ref.detach()) < 1e-6
    # The moments.  The C ABI takes b1 / b2 as float32 and the kernel forms 1 - b from them, torch forms 1 - b in double: the
    # rounding of float32(b), at most 2^-24 b, is magnified by 1 / (1 - b) in the weight of the new gradient -- a relative 5.4e-7
    # for m (b1 = 0.9) and 6.0e-5 for v (b2 = 0.999; float32(0.999) gives 1.3e-5) -- plus 16 fp32 roundings over the three steps.
    u = 2.0 ** -24
    assert rel_err(m, opt.state[p_ref]['exp_avg']) < u * 0.9 / 0.1 + 16 * u
    assert rel_err(v, opt.state[p_ref]['exp_avg_sq']) < u * 0.999 / 0.001 + 16 * u


def _head_reference(hd, E, eps_z, eps_t, R, Ho, zd, refine, theta_prior, normal, spacing):
    """Torch restatement of the head through the oracle (encoder tail + posterior_pool_kl)."""
    B = E.shape[0]
    hv = hd.view(3 + 2 * zd, B, R, Ho, Ho)
    p_r = torch.from_numpy(O.rotation_log_prior(R, refine, theta_prior, normal)).view(R, 1, 1)
    attn = hv[0] + p_r
    q = F.log_softmax(attn.reshape(B, -1), 1).view(B, R, Ho, Ho)
    a = F.softmax(attn.reshape(B, -1) - torch.log(E), 1).view(B, R, Ho, Ho)
    theta = hv[1:3].permute(1, 0, 2, 3, 4)
    offs = torch.from_numpy(O.rotation_offsets(R)) if refine else torch.zeros(R)
    if refine:
        theta = torch.stack((theta[:, 0] + offs.view(1, R, 1, 1), theta[:, 1]), 1)
    zv = hv[3:].permute(1, 0, 2, 3, 4)
    x = torch.zeros(B, 4, 2)
    z, th, dx, _, kl = O.posterior_pool_kl(x, attn, q, p_r, a, offs, theta, zv, spacing, eps_z, eps_t, R, theta_prior)
    return attn, q, a, z, th, dx.view(B, 2), kl


@pytest.mark.parametrize('R,Ho,zd,refine,normal,scale', [(8, 17, 2, True, False, 1.0), (4, 9, 3, False, False, 4.0),
                                                         (16, 5, 2, True, True, 8.0), (8, 33, 2, True, False, 30.0),
                                                         # few images x many positions: the chunked (several workgroups
                                                         # per image) kernels, R*P = 17 424 / 34 848
                                                         (16, 33, 5, True, False, 6.0), (8, 66, 2, True, False, 20.0)])
def test_attn_head(R, Ho, zd, refine, normal, scale):
    from tvae import ops
    B = 3
    RP = R * Ho * Ho
    theta_prior = math.pi / 4 if normal else math.pi
    spacing = 2.0 / 27
    hd = rnd(3 + 2 * zd, B * RP, seed=1, scale=0.5)
    hd[0] *= scale                                       # peaked attention for large scale (forces exp(q)==0)
    g = torch.Generator().manual_seed(2)
    E = torch.empty(B, RP).exponential_(generator=g)
    eps_z, eps_t = rnd(B, zd, seed=3), rnd(B, seed=4)
    hr = hd.clone().requires_grad_(True)
    ref = _head_reference(hr, E, eps_z, eps_t, R, Ho, zd, refine, theta_prior, normal, spacing)
    tb = ops.HeadTables(R, Ho, spacing, refine, theta_prior, normal, dev())
    hg = hd.clone().to(dev()).requires_grad_(True)
    got = ops.HeadFn.apply(hg, E.to(dev()), eps_z.to(dev()), eps_t.to(dev()), tb, B, zd)
    names = ['attn', 'q', 'a', 'z', 'theta', 'dx', 'kl']
    for nm, r_, g_ in zip(names, ref, got):
        assert rel_err(g_.reshape(-1), r_.reshape(-1)) < 5e-5, nm
    ws = [rnd(*r_.shape, seed=20 + i) for i, r_ in enumerate(ref)]
    coef = [0.3, 0.2, 5.0, 1.0, 1.0, 1.0, 1.0]
    sum(c * (r_ * w.to(r_.dtype)).sum() for c, r_, w in zip(coef, ref, ws)).backward()
    sum(c * (g_ * w.to(dev()).view_as(g_)).sum() for c, g_, w in zip(coef, got, ws)).backward()
    assert rel_err(hg.grad, hr.grad) < 2e-4


@pytest.mark.parametrize('fourier,zd,F_,B', [pytest.param(False, 2, 64, 2, id='False-2-64'), pytest.param(True, 3, 32, 2, id='True-3-32'),
                                             pytest.param(False, 3, 16, 40, id='False-3-16-B40')])
def test_decoder_ends(fourier, zd, F_, B):
    """dec_l0 / latent / fourier kernels against torch.  B = 40, F = 16: B zd > F zd, the other half of latent_bwd's index space,
    and more images than one round of its slices."""
    Np = 50
    Nt = B * Np
    xr = (torch.rand(B, Np, 2, generator=torch.Generator().manual_seed(1)) * 2 - 1)
    z = rnd(B, zd, seed=2)
    Wl = rnd(F_, zd, seed=3)
    LB = torch.empty(B, F_, device=dev())
    call('tvae_latent_bias', Wl.to(dev()), z.to(dev()), LB, B, F_, zd)
    assert rel_err(LB, z.double() @ Wl.double().t()) < TOL
    if not fourier:
        Wc, bc = rnd(F_, 2, seed=4), rnd(F_, seed=5)
        h = torch.empty(F_, Nt, device=dev())
        call('tvae_dec_l0_fwd', xr.to(dev()), Wc.to(dev()), bc.to(dev()), LB, h, Nt, F_, Nt, Np, 1, SLOPE)
        ref = F.leaky_relu(xr.view(Nt, 2).double() @ Wc.double().t() + bc.double() +
                           (z.double() @ Wl.double().t()).repeat_interleave(Np, 0), SLOPE).t()
        assert rel_err(h, ref) < TOL
    else:
        Ff, sigma = 48, 2.0 / 27
        Wf = rnd(Ff, 2, seed=6)
        bf = torch.rand(Ff, generator=torch.Generator().manual_seed(7)) * 2 * math.pi
        feat = torch.empty(Ff, Nt, device=dev())
        call('tvae_fourier_fwd', xr.to(dev()), Wf.to(dev()), bf.to(dev()), sigma, feat, Nt, Ff, Nt)
        x64 = xr.view(Nt, 2).double().requires_grad_(True)
        w32 = (Wf / torch.tensor(sigma, dtype=torch.float32)).double()
        ref = torch.cos(x64 @ w32.t() + bf.double())
        assert rel_err(feat, ref.t()) < 5e-5
        g = rnd(Ff, Nt, seed=8)
        (ref.t() * g.double()).sum().backward()
        gx = torch.empty(Nt, 2, device=dev())
        call('tvae_fourier_bwd', xr.to(dev()), Wf.to(dev()), bf.to(dev()), sigma, g.to(dev()), Nt, Ff, Nt, gx)
        assert rel_err(gx, x64.grad) < 5e-5
    S = rnd(B, F_, seed=9)
    dWl = torch.empty(F_, zd, device=dev())
    dz = torch.empty(B, zd, device=dev())
    call('tvae_latent_bwd', S.to(dev()), Wl.to(dev()), z.to(dev()), dWl, dz, B, F_, zd)
    assert rel_err(dWl, S.double().t() @ z.double()) < TOL
    assert rel_err(dz, S.double() @ Wl.double()) < TOL


def test_implicit_wgrad_and_multi_tile_dft_fp64():
    """Weight gradient with the implicit gradient operand over several reduction steps per slice, and the
    frequency-domain convolution on a batch whose (image, row) columns span several tiles: fp64 comparison."""
    from tvae._lib import query
    def rel(a, b):
        a, b = a.double().cpu(), b.double().cpu()
        return float((a - b).norm() / b.norm())
    g = torch.Generator().manual_seed(3)
    # weight gradient, several reduction steps per slice, implicit gradient operand
    M, N, K = 512, 20000 // 16 * 16, 384
    H = torch.randn(M, N, generator=g).clamp(-0.9, 0.9); X = torch.randn(K, N, generator=g)
    wo = torch.randn(M, generator=g); gy = torch.randn(N, generator=g)
    dW = torch.empty(M, K, device=dev()); ws = torch.empty(1 << 26, device=dev())       # >= tvae_linear_wgrad_x6_ws_floats(M, N, K): slices x M x K
    call('tvae_linear_wgrad_x6', H.to(dev()), X.to(dev()), dW, ws, ws.numel(), M, N, K, N, N, 0, vg_wo=wo.to(dev()),
         vg_gy=gy.to(dev()), vg_act=1, vg_slope=0.01, parts=3)
    d = wo.double()[:, None] * gy.double()[None, :] * torch.where(H.double() > 0, 1.0, 0.01)
    e1 = rel(dW, d @ X.double().t())
    # frequency-domain convolution, forward + weight gradient, a batch whose (image, row) columns span several tiles
    B, Cin, n, k, pad, C, R = 12, 1, 64, 64, 16, 32, 8
    Ho = n + 2 * pad - k + 1
    y = torch.rand(B, Cin, n, n, generator=g); bank = torch.randn(C * R, k * k, generator=g) * 0.02; bias = torch.randn(C, generator=g)
    at = torch.zeros(query('tvae_conv1_dft_at_floats', B, Cin, n, k, pad, C, R), device=dev())
    wsd = torch.empty(query('tvae_conv1_dft_ws_floats', B, Cin, n, k, pad, C, R), device=dev())
    out = torch.empty(C, B * R * Ho * Ho, device=dev())
    call('tvae_conv1_fwd_dft', y.to(dev()), bank.to(dev()), bias.to(dev()), out, at, wsd, wsd.numel(), B, Cin, n, k, pad, C, R, 0, 0.01, 3)
    ref = torch.nn.functional.conv2d(y.double(), bank.double().view(C * R, Cin, k, k), padding=pad).view(B, C, R, Ho, Ho) + bias.double().view(1, C, 1, 1, 1)
    e2 = rel(out.view(C, B, R, Ho, Ho).permute(1, 0, 2, 3, 4), ref)
    gg = torch.randn(B, C, R, Ho, Ho, generator=g)
    dbank = torch.empty(C * R, k * k, device=dev()); dbias = torch.empty(C, device=dev())
    call('tvae_conv1_wgrad_dft', gg.permute(1, 0, 2, 3, 4).contiguous().view(C, -1).to(dev()), at, dbank, dbias, wsd, wsd.numel(),
         B, Cin, n, k, pad, C, R, 3)
    refg = torch.nn.grad.conv2d_weight(y.double(), (C * R, Cin, k, k), gg.double().view(B, C * R, Ho, Ho), padding=pad)
    e3 = rel(dbank.view(C * R, Cin, k, k), refg)
    torch.cuda.synchronize()

    assert max(e1, e2, e3) < GEMM_TOL['f32'], (e1, e2, e3)


@pytest.mark.parametrize('N,nh,act,parts', [(4096, 103, 1, 2), (1000, 8, 1, 2), (2080, 23, 1, 2), (4128, 128, 1, 2), (999, 64, 2, 2),
                                            (1024, 65, 0, 2), (4096, 103, 1, 1)])
def test_enc_tail_wide(N, nh, act, parts):
    """Round 6: the encoder tail with 8 .. 128 head rows (galaxy: z_dim = 50 -> 103 rows; reference src/models.py:347-358,
    390-392) as two chained split-pipe GEMMs per direction -- tvae_enc_tail_fwd_wide / tvae_enc_tail_dgrad_wide against
    float64: H, the head rows, the sign words, dH and dA1; ragged N (not a multiple of the 32-column chunk), head-row counts
    that leave partial k-steps (nh % 16 != 0) and partial row tiles, a row of every operand 2^-20 below the rest (h3: per
    row relative error), and the bf16 throughput arithmetic at its own tolerance."""
    from tvae._lib import query
    C = 128
    s = 2.0 ** -20
    W2, b2 = rnd(C, C, seed=1, scale=C ** -0.5), rnd(C, seed=2)
    Wh, bh = rnd(nh, C, seed=3, scale=C ** -0.5), rnd(nh, seed=4)
    A1 = rnd(C, N, seed=5)
    W2[5] *= s; b2[5] *= s                                # a row of W2 (row of H), a head row, a column of Wh (row of dH)
    Wh[nh - 2] *= s; bh[nh - 2] *= s
    Wh[:, 19] *= s
    perm = _enc_tail_perm().cpu()
    split = 'tvae_dense_split2h' if parts == 2 else 'tvae_dense_split3'

    def cells(W, rows, K, transpose):
        a3 = torch.empty(query('tvae_dense_x6_bytes', rows, K) // 4, device=dev())
        call(split, W.contiguous().to(dev()), W.shape[1], a3, a3.numel() * 4, rows, K, transpose, None, None)
        return a3

    a1max = A1.abs().amax(dim=1).contiguous().to(dev()) if parts == 2 else None
    w3, whp = cells(W2, C, C, 0), cells(Wh[:, perm], nh, C, 0)
    H = torch.full((C, N), float('nan'), device=dev())
    heads = torch.full((nh, N), float('nan'), device=dev())
    bits = torch.zeros(2, N, 4, dtype=torch.int32, device=dev()) if act == 1 else None
    call('tvae_enc_tail_fwd_wide', w3, whp, A1.to(dev()), N, b2.to(dev()), bh.to(dev()), nh, H, N, heads, N,
         bits[0] if bits is not None else None, bits[1] if bits is not None else None, C, N, act, SLOPE, parts, a1max)
    Hr = act_ref(W2.double() @ A1.double() + b2.double()[:, None], act)
    hr = Wh.double() @ Hr + bh.double()[:, None]
    tol = ROW_TOL if parts == 2 else 2e-2
    assert row_rel_err(H, Hr) < tol
    assert row_rel_err(heads, hr) < (tol if parts == 2 else 3e-2)
    # inference form: no H, no sign words, the same head rows bit for bit
    h2 = torch.full((nh, N), float('nan'), device=dev())
    call('tvae_enc_tail_fwd_wide', w3, whp, A1.to(dev()), N, b2.to(dev()), bh.to(dev()), nh, None, N, h2, N, None, None, C, N,
         act, SLOPE, parts, a1max)
    assert torch.equal(h2, heads)
    if act != 1:
        return
    # sign words: bit (row & 31) of word (row >> 5) of column n (the layout tvae_enc_tail_fwd_x6 writes)
    Hs = H.double().cpu()
    for t, ref in ((bits[0], Hs), (bits[1], A1.double())):
        w = t.cpu().numpy().astype(np.uint32)             # [N][4]
        got = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(N, 128).T
        assert np.array_equal(got.astype(bool), (ref > 0).numpy())
    dheads = rnd(nh, N, seed=6)
    dheads[3] *= s
    dmax = dheads.abs().max().reshape(1).to(dev()) if parts == 2 else None
    wht, w3p = cells(Wh, C, nh, 1), cells(W2.t()[:, perm], C, C, 0)
    dH = torch.full((C, N), float('nan'), device=dev())
    dA1 = torch.full((C, N), float('nan'), device=dev())
    call('tvae_enc_tail_dgrad_wide', wht, w3p, dheads.to(dev()), N, nh, bits[0], bits[1], dH, N, dA1, N, C, N, SLOPE, parts, dmax)
    dHr = (Wh.double().t() @ dheads.double()) * dact_ref(Hs, 1)
    dAr = (W2.double().t() @ dHr) * dact_ref(A1.double(), 1)
    assert row_rel_err(dH, dHr) < tol
    assert row_rel_err(dA1, dAr) < tol
    # without the dH output: the same dA1 bit for bit
    dA2 = torch.full((C, N), float('nan'), device=dev())
    call('tvae_enc_tail_dgrad_wide', wht, w3p, dheads.to(dev()), N, nh, bits[0], bits[1], None, N, dA2, N, C, N, SLOPE, parts, dmax)
    assert torch.equal(dA2, dA1)
    with pytest.raises(Exception):                       # more head rows than the kernel's 128
        call('tvae_enc_tail_fwd_wide', w3, whp, A1.to(dev()), N, b2.to(dev()), bh.to(dev()), 129, H, N, heads, N, None, None, C, N,
             act, SLOPE, parts, a1max)
    if parts == 2:
        with pytest.raises(Exception):                   # h3 without the operand bound
            call('tvae_enc_tail_dgrad_wide', wht, w3p, dheads.to(dev()), N, nh, bits[0], bits[1], dH, N, dA1, N, C, N, SLOPE, 2, None)


def test_rowdot_seg_amax():
    """tvae_rowdot_seg's optional by-product (ABI 7): max |X| into a zeroed word, next to the segment sums."""
    M, N = 9, 70001
    X = rnd(M, N, seed=3)
    X[4, 12345] = -77.5
    tmp = torch.empty(35, M, device=dev())
    amax = torch.zeros(1, device=dev())
    call('tvae_rowdot_seg', X.to(dev()), N, None, 1, M, N, 2048, tmp, amax)
    assert float(amax) == 77.5
    assert rel_err(tmp.sum(0), X.double().sum(1)) < 1e-5


@pytest.mark.parametrize('sigma,span,amin', [(2.0 / 127, 2.0, 300.0), (0.2 / 127, 2.0, 3000.0), (0.01, 1.5, 300.0), (2.0 / 27, 1.0, 30.0)])
def test_fourier_bwd_large_arguments(sigma, span, amin):
    """tvae_fourier_bwd evaluates sin with v_sin_f32 after its own range reduction.  Against float64 at the galaxy
    sigma with |coordinates| ~ 2 (|arg| up to ~500 rad), at a 10x smaller sigma (~5 000 rad: far outside the instruction's native
    +-256 revolutions), and at the dsprites default 0.01 (reference train_dsprites.py:492-494).  The float64 reference takes
    the fp32-ROUNDED argument (what any fp32 forward, the reference's included, evaluates cos of)."""
    Nt, Ff = 4096, 256
    xr = (torch.rand(Nt, 2, generator=torch.Generator().manual_seed(1)) * 2 - 1) * span
    Wf, bf = rnd(Ff, 2, seed=2), torch.rand(Ff, generator=torch.Generator().manual_seed(3)) * 2 * math.pi
    g = rnd(Ff, Nt, seed=4)
    gx = torch.empty(Nt, 2, device=dev())
    call('tvae_fourier_bwd', xr.to(dev()), Wf.to(dev()), bf.to(dev()), sigma, g.to(dev()), Nt, Ff, Nt, gx)
    w = (Wf / sigma)                                      # fp32, as the kernel forms it
    arg = (xr[:, 0:1] * w[:, 0][None, :] + xr[:, 1:2] * w[:, 1][None, :] + bf[None, :])      # [Nt][Ff] fp32
    assert float(arg.abs().max()) > amin
    t = -torch.sin(arg.double()) * g.double().t()
    ref = torch.stack([(t * w[:, 0].double()[None, :]).sum(1), (t * w[:, 1].double()[None, :]).sum(1)], 1)
    # per element: rounding of the fp32 argument sum (up to 3 ulp of |arg|) times the slope of sin, summed over Ff features
    tol = 4e-7 * float(arg.abs().max()) + 2e-6
    assert rel_err(gx, ref) < tol, (rel_err(gx, ref), tol)


@pytest.mark.timeout(900)
@pytest.mark.parametrize('var', ['TVAE_DFT_FULL_FRAME', 'TVAE_DFT_YSPECTRAL'])
def test_conv1_dft_alternative_formulations(var):
    """The two round-4 formulations of the frequency-domain convolution that the library still carries behind a switch -- the
    reference's full zero-padded frame n + 2 pad (its own ring instances 4-6) and the transform along BOTH axes -- run the whole
    fp64 comparison above in a process of their own (the switches are read once per process).  This test is what keeps them
    alive (every remaining switch names its test)."""
    import subprocess
    import sys
    env = dict(os.environ, **{var: '1'})
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-k', 'conv1_dft_matches_fp64',
                        '-p', 'no:cacheprovider'], env=env, capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout


@pytest.mark.parametrize('M,K', [(512, 384), (1024, 512)])
@pytest.mark.parametrize('parts', [3, 2, 1])
def test_linear_x6_lean_store_epilogue_and_measured_maximum(M, K, parts):
    """Round 6: plain hidden-layer launches that store their output take the lean store epilogue (dense_x6_kernel<0, NP, 3>: whole
    512-row tiles -- one and two row tiles here) and can leave max |stored value| in a zeroed word (y_amax, ABI 7): forward with
    bias + LeakyReLU and without activation, data gradient under the LeakyReLU mask of a saved activation, in all three split
    arithmetics against float64; the word must hold EXACTLY the maximum of what was stored."""
    from tvae._lib import query
    N = 640
    W, X, b = rnd(M, K, seed=1, scale=K ** -0.5), rnd(K, N, seed=2), rnd(M, seed=3)
    split = 'tvae_dense_split2h' if parts == 2 else 'tvae_dense_split3'
    tol = {3: GEMM_TOL['f32'], 2: GEMM_TOL['f32'], 1: 2e-2}[parts]

    def cells(Wm, rows, Kk, tr):
        a3 = torch.empty(query('tvae_dense_x6_bytes', rows, Kk) // 4, device=dev())
        call(split, Wm.to(dev()), Wm.shape[1], a3, a3.numel() * 4, rows, Kk, tr, None, None)
        return a3

    xmax = X.abs().max().reshape(1).to(dev()) if parts == 2 else None
    w3 = cells(W, M, K, 0)
    for act in (1, 0):
        Y = torch.full((M, N), float('nan'), device=dev())
        amax = torch.zeros(1, device=dev())
        call('tvae_linear_fwd_x6', w3, X.to(dev()), b.to(dev()), None, Y, M, N, K, N, N, act, SLOPE, parts=parts, x_amax=xmax,
             y_amax=amax)
        ref = act_ref(W.double() @ X.double() + b.double()[:, None], act)
        assert rel_err(Y, ref) < tol
        assert float(amax) == float(Y.abs().max())
    d = rnd(K, N, seed=6)                                 # gradient of this layer's OUTPUT rows ... transposed problem: rows = K
    aux = rnd(M, N, seed=7).clamp(-0.9, 0.9)
    # dX[m][n] = act'(aux[m][n]) * sum_k Wt[k][m] d[k][n] with Wt = W^T (K x M): reuse W as the (K = rows of d) x (M = outputs) weight
    Wt = rnd(K, M, seed=8, scale=K ** -0.5)
    w3t = cells(Wt, M, K, 1)
    dmax = d.abs().max().reshape(1).to(dev()) if parts == 2 else None
    dX = torch.full((M, N), float('nan'), device=dev())
    amax = torch.zeros(1, device=dev())
    call('tvae_linear_dgrad_x6', w3t, d.to(dev()), None, aux.to(dev()), dX, K, N, M, N, N, 1, SLOPE, parts=parts, x_amax=dmax,
         y_amax=amax)
    refg = (Wt.double().t() @ d.double()) * dact_ref(aux.double(), 1)
    assert rel_err(dX, refg) < tol
    assert float(amax) == float(dX.abs().max())
    with pytest.raises(Exception):                       # y_amax needs a stored output with nothing fused behind it
        call('tvae_linear_fwd_x6', w3, X.to(dev()), b.to(dev()), None, None, M, N, K, N, N, 1, SLOPE, parts=parts, x_amax=xmax,
             y_amax=amax)


# ---- the guard itself on the real library, and the entry points no other test of this file reaches --------------------------
def test_guard_reports_a_planted_one_word_overrun():
    """Positive control of tests/guardband.py on the real library: tvae_seg_sum is told L outputs but given a VIEW of L - 1 of a
    tensor that has L.  Unguarded the call is legal (every address lies in the caller's own tensor); guarded, the last store
    falls into the band behind `out`, and the report has to say exactly that: one word, offset 0, argument 3."""
    from tvae import _lib
    S, L = 5, 300
    X = rnd(S, L, seed=1).to(dev())
    full = torch.zeros(L, device=dev())
    short = full[:L - 1]
    with pytest.raises(guardband.GuardViolation) as ei:
        with guardband.GuardedCalls():
            call('tvae_seg_sum', X, S, L, short, 1.0, 0)
    (v,) = ei.value.violations
    assert (v['entry'], v['kind'], v['args'], v['side'], v['count'], v['first'], v['last']) == \
        ('tvae_seg_sum', 'band', (3,), 'behind', 1, 0, 0), v
    assert v['scalars'] == {1: S, 2: L, 4: 1.0, 5: 0} and 'tvae_seg_sum' in str(ei.value)
    ref = X.double().sum(0)
    assert rel_err(short, ref[:L - 1]) < TOL and float(full[L - 1]) == 0.0     # the interior came back, nothing else did
    old = _lib.set_call_hook(None)
    try:
        call('tvae_seg_sum', X, S, L, short, 1.0, 0)
    finally:
        _lib.set_call_hook(old)
    assert rel_err(full, ref) < TOL


@pytest.mark.parametrize('B', [1, 3, 256, 257, 1000])
def test_elbo_reduce(B):
    """tvae_elbo_reduce / _bwd.  The kernel sums in double: kld within 1e-12 of the exact mean (B 2^-53 << 1e-12), logp within one
    float32 ulp of float32(exact mean), elbo == double(logp) - kld exactly from the returned values.  Backward: the eight
    NULL / non-NULL combinations of the upstream gradients, every element exactly float32((g_elbo + g_logp) / B) resp.
    float32((g_kld - g_elbo) / B)."""
    g = torch.Generator().manual_seed(100 + B)
    lp = -700.0 + 50.0 * torch.randn(B, generator=g)
    kl = 10.0 + 3.0 * torch.randn(B, generator=g)
    elbo = torch.empty((), dtype=torch.float64, device=dev())
    logp = torch.empty((), dtype=torch.float32, device=dev())
    kld = torch.empty((), dtype=torch.float64, device=dev())
    call('tvae_elbo_reduce', lp.to(dev()), kl.to(dev()), B, elbo, logp, kld)
    kl_ref = math.fsum(kl.double().tolist()) / B
    lp_ref = np.float32(math.fsum(lp.double().tolist()) / B)
    assert abs(kld.item() - kl_ref) <= 1e-12 * abs(kl_ref), (kld.item(), kl_ref)
    assert abs(float(logp.item()) - float(lp_ref)) <= float(np.spacing(np.abs(lp_ref))), (logp.item(), lp_ref)
    assert elbo.item() == float(logp.item()) - kld.item()
    ge, gl, gk = -1.25, 0.3, 2.5
    for combo in range(8):
        t_ge = torch.tensor(ge, dtype=torch.float64, device=dev()) if combo & 1 else None
        t_gl = torch.tensor(gl, dtype=torch.float32, device=dev()) if combo & 2 else None
        t_gk = torch.tensor(gk, dtype=torch.float64, device=dev()) if combo & 4 else None
        g_lp = torch.full((B,), float('nan'), device=dev())
        g_kl = torch.full((B,), float('nan'), device=dev())
        call('tvae_elbo_reduce_bwd', t_ge, t_gl, t_gk, B, g_lp, g_kl)
        e_, l_, k_ = ge if combo & 1 else 0.0, float(np.float32(gl)) if combo & 2 else 0.0, gk if combo & 4 else 0.0
        want_lp, want_kl = np.float32((e_ + l_) / B), np.float32((k_ - e_) / B)
        assert (g_lp.cpu().numpy() == want_lp).all() and (g_kl.cpu().numpy() == want_kl).all(), combo
    with pytest.raises(Exception):
        call('tvae_elbo_reduce', lp.to(dev()), kl.to(dev()), 0, elbo, logp, kld)
    with pytest.raises(Exception):
        call('tvae_elbo_reduce', lp.to(dev()), kl.to(dev()), B, elbo, None, kld)
    with pytest.raises(Exception):
        call('tvae_elbo_reduce_bwd', None, None, None, 0, g_lp, g_kl)
    with pytest.raises(Exception):
        call('tvae_elbo_reduce_bwd', None, None, None, B, g_lp, None)


@pytest.mark.parametrize('B,n,kc', [(3, 32, 31), (2, 32, 33), (5, 17, 5), (1, 40, 1), (2, 64, 63)])
def test_ctf_corr(B, n, kc):
    """Per-image cross-correlation with an odd filter (kc = 33 > n: the filter is larger than the image) against conv2d in
    float64; flip = 1 against autograd's gradient with respect to the input; and the two as adjoints of each other."""
    x, ctf, g = rnd(B, n * n, seed=1), rnd(B, kc * kc, seed=2, scale=1.0 / kc), rnd(B, n * n, seed=3)
    x64 = x.double().view(1, B, n, n).requires_grad_(True)
    ref = F.conv2d(x64, ctf.double().view(B, 1, kc, kc), padding=kc // 2, groups=B)
    (ref.view(B, -1) * g.double()).sum().backward()
    out = torch.full((B, n * n), float('nan'), device=dev())
    call('tvae_ctf_corr', x.to(dev()), ctf.to(dev()), out, B, n, kc, 0)
    assert rel_err(out, ref.detach().view(B, -1)) < TOL
    gi = torch.full((B, n * n), float('nan'), device=dev())
    call('tvae_ctf_corr', g.to(dev()), ctf.to(dev()), gi, B, n, kc, 1)
    assert rel_err(gi, x64.grad.view(B, -1)) < TOL
    lhs, rhs = float((out.double().cpu() * g.double()).sum()), float((x.double() * gi.double().cpu()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float(out.double().norm()) * float(g.double().norm()), (lhs, rhs)
    with pytest.raises(Exception):                 # an even filter has no centre (kc - 1: within the tensors given either way)
        call('tvae_ctf_corr', x.to(dev()), ctf.to(dev()), out, B, n, kc - 1, 0)


def _mask_margin(c, n, radius):
    """min over pixels of |d^2 - r^2| in float64 for the image centre c (2,), and the mask, on the reference's grid
    (train_particles.py:309-333: gx_j = -ceil(n/2) + j, gy_i = floor(n/2) - i)."""
    gx = torch.arange(n, dtype=torch.float64) - (n + 1) // 2
    gy = n // 2 - torch.arange(n, dtype=torch.float64)
    d2 = (c[0].double() - gx)[None, :] ** 2 + (c[1].double() - gy)[:, None] ** 2
    return float((d2 - radius * radius).abs().min()), (d2 < radius * radius).reshape(-1)


@pytest.mark.parametrize('n', [32, 33, 50])
@pytest.mark.parametrize('radius', [3.5, 7.25, 12.0, None])
def test_loglik_masked(n, radius):
    """tvae_loglik_masked_fwd / _bwd against oracle.particles_logp in float64 and its autograd gradient.  B = 4; for a finite
    radius the last image's centre lies outside the frame by more than the radius (lp == 0, no gradient); radius None = 4 n
    keeps every pixel and has to give exactly what tvae_loglik_fwd / _bwd (kind 1) give on the same data (same thread count,
    same order, same tree).  A pixel ON the circle is ill-conditioned (the kernel forms d^2 in fp32: rounding of a few 1e-5
    at d^2 ~ 150), so centres come from a seeded generator and are redrawn until no pixel has |d^2 - r^2| < 1e-3 in float64;
    of 20 candidate draws at most 2 may be rejected (2 pi 1e-3 ~ 0.6 % is expected), so the filter cannot select the
    cases away."""
    B, spacing = 4, 0.5                                  # a power of two: dx / spacing is exact in fp32 and in fp64
    r = 4.0 * n if radius is None else radius
    gen = torch.Generator().manual_seed(7 * n + int(10 * r))
    cand = torch.rand(20, 2, generator=gen) * 12 - 6
    ok = [_mask_margin(c, n, r)[0] >= 1e-3 for c in cand]
    assert ok.count(False) <= 2, ok
    centres = cand[[i for i, o in enumerate(ok) if o][:B]].clone()
    if radius is not None:
        centres[B - 1] = torch.tensor([n / 2 + r + 3.25, 1.5])
    masks = []
    for c in centres:                                    # the margin holds for the inputs that are used
        mg, mk = _mask_margin(c, n, r)
        assert mg >= 1e-3
        masks.append(mk)
    mask = torch.stack(masks)
    assert bool(mask.all()) == (radius is None) and (radius is None or not mask[B - 1].any())
    dx = (centres * spacing).float()
    yh, y, w = rnd(B, n * n, seed=1), rnd(B, n * n, seed=2), rnd(B, seed=3)
    yh64 = yh.double().requires_grad_(True)
    per = torch.stack([O.particles_logp(yh64[b:b + 1], y[b].double().view(1, 1, n, n), None, r, dx[b].double().view(1, 1, 2), spacing)
                       for b in range(B)])
    (per * w.double()).sum().backward()
    d = [t.to(dev()) for t in (yh, y, dx, w)]
    lp = torch.full((B,), float('nan'), device=dev())
    call('tvae_loglik_masked_fwd', d[0], d[1], d[2], 1.0 / spacing, r, B, n, lp)
    assert rel_err(lp, per.detach()) < TOL
    gyh = torch.full((B, n * n), float('nan'), device=dev())
    call('tvae_loglik_masked_bwd', d[0], d[1], d[2], 1.0 / spacing, r, B, n, d[3], gyh)
    assert rel_err(gyh, yh64.grad) < TOL
    assert torch.equal(gyh.cpu() != 0, mask)             # the zero pattern IS the reference's mask
    if radius is not None:
        assert float(lp[B - 1]) == 0.0 and not gyh[B - 1].any()
    else:
        lp1 = torch.full((B,), float('nan'), device=dev())
        g1 = torch.full((B, n * n), float('nan'), device=dev())
        call('tvae_loglik_fwd', d[0], d[1], lp1, B, n * n, 1)
        call('tvae_loglik_bwd', d[0], d[1], d[3], g1, B, n * n, 1)
        assert torch.equal(lp, lp1) and torch.equal(gyh, g1)


@pytest.mark.parametrize('R,Ho,zd,scale,tie', [(4, 5, 1, 1.0, False), (8, 17, 2, 1.0, False), (8, 17, 2, 1.0, True),
                                               (8, 66, 2, 30.0, False), (4, 9, 50, 1.0, False)])
def test_get_latent(R, Ho, zd, scale, tie):
    """tvae_get_latent against float64: argmax over (r, h, w) of logit + log p(r) (the sum itself in fp32, as the kernel and the
    reference form it; everything behind it in float64), gather of (z_mu, exp(z_logstd)) and theta there, softmax-expected grid
    position.  Fewer positions than the 1024 threads, 34 848 positions, z_dim 50, a padded row stride, logits x 30 (peaked
    softmax); tie: the maximum planted twice, at j1 < j2 with (j2 mod 1024) < (j1 mod 1024) -- thread order and index order
    disagree, the FIRST index has to win (include/tvae_hip.h)."""
    B, P = 3, Ho * Ho
    RP, nh = R * P, 3 + 2 * zd
    ldh = B * RP + 37
    heads = rnd(nh, ldh, seed=1)
    heads[0] *= scale
    heads[3 + zd:] *= 0.5
    p_r = torch.log_softmax(rnd(R, seed=2), 0)
    off, grid, tos = rnd(R, seed=3), rnd(P, 2, seed=4), 0.7
    j1, j2 = 1000, 1029
    if tie:
        assert j2 < RP and j1 // P == j2 // P and j2 % 1024 < j1 % 1024
        for b in range(B):
            heads[0, b * RP + j1] = heads[0, b * RP + j2] = 50.0
    zc = torch.full((B, 2 * zd), float('nan'), device=dev())
    th = torch.full((B, 1), float('nan'), device=dev())
    dxo = torch.full((B, 2), float('nan'), device=dev())
    call('tvae_get_latent', heads.to(dev()), ldh, p_r.to(dev()), off.to(dev()), grid.to(dev()), B, R, P, zd, tos, zc, th, dxo)
    zc_ref, th_ref, dx_ref = torch.empty(B, 2 * zd, dtype=torch.float64), torch.empty(B, 1, dtype=torch.float64), \
        torch.empty(B, 2, dtype=torch.float64)
    for b in range(B):
        l32 = heads[0, b * RP:(b + 1) * RP] + p_r.repeat_interleave(P)
        j = int((l32 == l32.max()).nonzero()[0])
        if tie:
            assert j == j1 and l32[j2] == l32[j1]
        col = heads[:, b * RP + j].double()
        zc_ref[b] = torch.cat([col[3:3 + zd], torch.exp(col[3 + zd:])])
        th_ref[b] = col[1] + tos * off[j // P].double()
        a = torch.softmax(l32.double(), 0).view(R, P).sum(0)
        dx_ref[b] = a @ grid.double()
    assert torch.equal(zc[:, :zd].cpu(), zc_ref[:, :zd].float())          # a gather: exact (and shows WHICH index won)
    assert rel_err(zc, zc_ref) < TOL and rel_err(th, th_ref) < TOL and rel_err(dxo, dx_ref) < TOL


@pytest.mark.parametrize('Mr,nparts', [(512, 3), (384, 3), (512, 2)])
def test_dgrad_rowsum_total(Mr, nparts):
    """tvae_dgrad_rowsum_total: tvae_linear_dgrad_x6 with rs_db = rs_dwo = NULL leaves only the per-tile partial sums; the total
    as a call of its own has to give bit for bit the rs_db / rs_dwo of the fused launch (same kernel, same partials), and both
    match float64 (the two-valued setups of test_linear_x6_implicit_gradient_operand / test_h3_decoder_entry_points)."""
    from tvae._lib import query
    N, K = 1024, 512
    W, H = rnd(Mr, K, seed=1, scale=Mr ** -0.5), rnd(Mr, N, seed=2).clamp(-0.9, 0.9)
    wo, gy = rnd(Mr, seed=3), rnd(N, seed=4)
    aux = rnd(K, N, seed=5).clamp(-0.9, 0.9)
    split = 'tvae_dense_split2h' if nparts == 2 else 'tvae_dense_split3'
    w3 = torch.empty(query('tvae_dense_x6_bytes', K, Mr) // 4, device=dev())
    cs = torch.empty(K, device=dev())
    call(split, W.to(dev()), K, w3, w3.numel() * 4, K, Mr, 1, wo.to(dev()), cs)
    gys = gy.sum().reshape(1).to(dev())
    Hd, auxd, gyd, wod = H.to(dev()), aux.to(dev()), gy.to(dev()), wo.to(dev())
    res = []
    for fused in (True, False):
        dX = torch.full((K, N), float('nan'), device=dev())
        part = torch.full(((N // 128) * Mr * 2,), float('nan'), device=dev())
        db, dwo = torch.full((Mr,), float('nan'), device=dev()), torch.full((Mr,), float('nan'), device=dev())
        call('tvae_linear_dgrad_x6', w3, Hd, None, auxd, dX, Mr, N, K, N, N, 1, SLOPE, vg_gy=gyd, vg_csum=cs, rs_part=part,
             rs_part_floats=part.numel(), rs_wo=wod, rs_gysum=gys, rs_db=db if fused else None, rs_dwo=dwo if fused else None,
             parts=nparts)
        if not fused:
            assert torch.isnan(db).all() and torch.isnan(dwo).all()
            call('tvae_dgrad_rowsum_total', part, N // 128, Mr, wod, gys, SLOPE, db, dwo, None, None)
        res.append((dX, part, db, dwo))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    _, _, db, dwo = res[1]
    assert rel_err(db, (wo.double()[:, None] * gy.double()[None, :] * dact_ref(H.double(), 1)).sum(1)) < TOL
    assert rel_err(dwo, H.double() @ gy.double()) < TOL
    with pytest.raises(Exception):
        call('tvae_dgrad_rowsum_total', part, N // 128, Mr, wod, gys, SLOPE, db, None, None, None)
    with pytest.raises(Exception):
        call('tvae_dgrad_rowsum_total', part, 0, Mr, wod, gys, SLOPE, db, dwo, None, None)


def test_every_entry_point_ran_under_guard(request):
    """Keeps the coverage closed: when this whole file has run in the session, every entry point of the C ABI
    (tvae._lib.SIGNATURES) has been called under guard bands by some test of it.  No exemptions."""
    from tvae import _lib
    mine = [it for it in request.session.items if it.fspath == request.node.fspath]
    ran = {getattr(it, 'originalname', None) or it.name for it in mine}
    defined = {k_ for k_, v_ in globals().items() if k_.startswith('test_') and callable(v_)}
    tr = request.config.pluginmanager.get_plugin('terminalreporter')
    cut = [it for it in (tr.stats.get('deselected', []) if tr else []) if getattr(it, 'fspath', None) == request.node.fspath]
    if ran != defined or cut:
        pytest.skip('only meaningful when the whole file runs (a -k / -m / node-id selection left part of it out)')
    # ('stand_in' is the Python stand-in of the guard's CPU self-tests, when they ran in the same session)
    assert guardband.GUARDED_NAMES - {'stand_in'} == set(_lib.SIGNATURES), \
        (sorted(set(_lib.SIGNATURES) - guardband.GUARDED_NAMES), sorted(guardband.GUARDED_NAMES - set(_lib.SIGNATURES)))
