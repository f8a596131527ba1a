"""float64 restatement of the coordinate transform x' = (x - dx) R(theta) (tvae.ops.CoordFn: coord_fwd_kernel, coord_bwd_kernel)
with the condition quantities of its error bounds, and the cases both test_head_ref_cpu.py (which measures K on fp32 CPU
arithmetic) and test_coord_fp64_gpu.py run.  A plain helper module.

    x'_0 = X_0 c - X_1 s,  x'_1 = X_0 s + X_1 c,   X = x - dx,  c = cos theta, s = sin theta
    d dx_0 = -sum_p (g_0 c + g_1 s),  d dx_1 = sum_p (g_0 s - g_1 c),  d theta = sum_p (g_1 x'_0 - g_0 x'_1)

Condition quantities (u = 2^-24).  cosf / sinf at |theta| <= 20 are within a few u of 1 in ABSOLUTE terms (the argument
reduction does not keep the relative error of a value near a zero crossing), so |c| and |s| count as 1:
    forward, per element:        m_p = |x_0| + |dx_0| + |x_1| + |dx_1|
    d dx, per image, component:  sum_p (|g_0| + |g_1|)
    d theta, per image:          sum_p (|g_0| + |g_1|) m_p
K: fp32 torch on the CPU (the expression of test_hip_primitives.py::test_coord and its autograd) against this file,
8 x the worst ratio and not below 16 (test_head_ref_cpu.py::test_coord_budget_constants)."""
import numpy as np
import torch

U = 2.0 ** -24
# measured ratios: forward 2.79 (K = 8 x 2.79 = 22.3, kept as 23), dx 0.39, theta 0.57 (K = 16, the floor)
K = {'fwd': 23.0, 'dx': 16.0, 'theta': 16.0}

# Np: 81 = 9 x 9 (fewer than the 256 threads of the backward's workgroup), 784 = 28 x 28 (a fourth trip, partly filled),
# 33 x 31 (not square), 4096 + 37 (seventeen trips, the last one short; free coordinates).
# B: 1, 3, 300; and B = 2675 at Np = 784: 2 097 200 elements, 48 more than the 8192 x 256 threads grid1d allows the forward --
# the second round of its grid-stride loop (B = 300 stays within one round: 235 200 elements).
NPS = [81, 784, 33 * 31, 4096 + 37]
CASES = [(B, Np) for Np in NPS for B in (1, 3, 300)] + [(2675, 784)]


def case(B, Np):
    """-> xc [Np][2], dx [B][2] in +-1, theta [B] in +-20 rad, g [B][Np][2]; fp32."""
    from tvae import tables
    gen = torch.Generator().manual_seed(1000 * B + Np)
    if Np == 33 * 31:
        xc = torch.from_numpy(tables.image_coords(33, 31))
    elif int(np.sqrt(Np)) ** 2 == Np:
        xc = torch.from_numpy(tables.image_coords(int(np.sqrt(Np))))
    else:
        xc = torch.rand(Np, 2, generator=gen) * 2 - 1
    dx = torch.rand(B, 2, generator=gen) * 2 - 1
    th = (torch.rand(B, generator=gen) * 2 - 1) * 20.0
    g = torch.randn(B, Np, 2, generator=gen)
    return xc.contiguous(), dx, th, g


def transform(xc, dx, th):
    """The expression of test_coord, in the dtype of its arguments."""
    x = xc.expand(th.shape[0], -1, -1) - dx.unsqueeze(1)
    rot = torch.stack([torch.stack([torch.cos(th), torch.sin(th)], 1), torch.stack([-torch.sin(th), torch.cos(th)], 1)], 1)
    return torch.bmm(x, rot)


def reference(xc, dx, th, g):
    """-> (x' [B][Np][2], d dx [B][2], d theta [B]) float64 and their condition quantities (same shapes)."""
    dx64, th64 = dx.double().requires_grad_(True), th.double().requires_grad_(True)
    xr = transform(xc.double(), dx64, th64)
    (xr * g.double()).sum().backward()
    m = (xc.double().abs().sum(1)[None, :] + dx.double().abs().sum(1)[:, None])          # [B][Np]
    ga = g.double().abs().sum(2)                                                         # [B][Np]
    cond = (m.unsqueeze(2).expand(-1, -1, 2), ga.sum(1, keepdim=True).expand(-1, 2), (ga * m).sum(1))
    return (xr.detach(), dx64.grad, th64.grad), cond


def ratios(got, ref, cond):
    """Worst error / (u condition) of (x', d dx, d theta)."""
    return {n_: float(((torch.as_tensor(g_).detach().double().cpu() - r_).abs() / (U * c_)).max())
            for n_, g_, r_, c_ in zip(K, got, ref, cond)}
