"""float64 restatements of the streaming kernels at the two ends of the MLPs (csrc/small_kernels.hpp, fused_tail_kernels.hpp
behind abi_small.hip): tvae_rowdot_seg, tvae_seg_sum, tvae_coldot, tvae_outer_mask, tvae_act_bwd, tvae_dec_l0_fwd,
tvae_latent_bias, tvae_latent_bwd, tvae_fourier_fwd / _bwd, tvae_dec_out_bwd, tvae_dec_in_bwd, tvae_heads_fwd / _bwd -- with the
condition quantities of their error bounds and the cases both test_mlp_ends_ref_cpu.py (which measures K on fp32 CPU
arithmetic) and test_mlp_ends_fp64_gpu.py run.  A plain helper module.

Every operation is ONE expression, written in the dtype `dt` of the call: float64 is the reference, float32 on the CPU is what
K is measured with, and cond=True evaluates the same expression on the absolute values of its operands -- the per-element
CONDITION QUANTITY, the sum of the absolute values of the terms the fp32 kernel adds.  A kernel result `got` has to satisfy

    |got - ref| <= K[name] * U * cond  (+ floor, tvae_fourier_bwd only),     U = 2^-24, every element.

Activation derivative, from the STORED output y (act_deriv_from_out): act 0: 1; leaky ReLU: y > 0 ? 1 : slope -- slope at +0.0
and at -0.0; tanh: 1 - y y, whose condition quantity is 1 + y y (the two terms of the difference: at |y| within an ulp of 1 the
fp32 result keeps no correct digit of 1 - y y, and the bound says so).  H / X / Y of the backward kernels carry SPECIALS at
plant_columns(): first and last column of a panel, last valid column of a ragged float4, ...

Fourier features: w = fp32(Wf / sigma) and the argument a = fp32(x0 w0 + x1 w1 + b) as fp32 torch rounds it; the reference is the
float64 cosine / sine of THAT argument.  A kernel may round the argument differently (fused multiply-adds), so the condition
quantity has a second part A |slope|, A = |x0 w0| + |x1 w1| + |b|: forward |cos a| + A |sin a|, backward per term
(|sin a| + A |cos a|) |g| |w_j|.  The backward evaluates the sine with the hardware instruction after its own range reduction:
FOURIER_SIN_ABS = 2e-6 absolute per term (the floor of test_hip_primitives.py::test_fourier_bwd_large_arguments; nothing on the
CPU can measure it) is added to its bound as floor = 2e-6 sum_f |g| |w_j|.  What an MI355X showed of it: FOURIER_SIN_SEEN
below; the number is not tightened from it.

First decoder layer: pre = w0 x0 + w1 x1 + bc + lb with condition c = the same on absolute values; h = act(pre) has the
condition |h| + c L, L the local Lipschitz constant of act (leaky ReLU: 1 unless pre < -64 U c, where the sign is certain, then
slope; tanh: 1 - tanh^2).

K: fp32 torch on the CPU against this file on every case below, K = max(16, 8 x worst ratio)
(test_mlp_ends_ref_cpu.py::test_budget_constants measures and prints them):

    output       ratio   8 x     K      output       ratio   8 x     K      output       ratio   8 x     K
    rowdot       3.425  27.40   28      latent_bias  1.697  13.58   16      in_gxr       3.072  24.58   25
    seg_sum      1.499  11.99   16      dWl          1.803  14.42   16      in_Simg      1.493  11.94   16
    coldot       3.822  30.58   31      dz           2.102  16.81   17      in_dbc       0.136   1.09   16
    outer_mask   2.749  22.00   23      fourier_fwd  0.576   4.61   16      in_dWc       0.918   7.34   16
    act_bwd      1.404  11.23   16      fourier_bwd  0.767   6.14   16      heads_Y      5.176  41.40   42
    dec_l0       1.224   9.79   16      out_D        2.701  21.61   22      heads_dX     3.319  26.55   27
                                        out_tot      1.154   9.23   16      heads_tot    1.170   9.36   16
"""
import functools
import itertools
import math

import torch
import torch.nn.functional as F_

U = 2.0 ** -24
SLOPE = float(torch.tensor(0.01, dtype=torch.float32))       # what the kernels get: fp32(0.01)
FOURIER_SIN_ABS = 2e-6
SENTINEL = -7777.0            # prefill of strided outputs: pad columns must come back holding it
PAD_IN = 1e30                 # pad columns of strided inputs: a read of one shows in the result
F64, F32 = torch.float64, torch.float32

K = {'rowdot': 28.0, 'seg_sum': 16.0, 'coldot': 31.0, 'outer_mask': 23.0, 'act_bwd': 16.0, 'dec_l0': 16.0,
     'latent_bias': 16.0, 'dWl': 16.0, 'dz': 17.0, 'fourier_fwd': 16.0, 'fourier_bwd': 16.0, 'out_D': 22.0, 'out_tot': 16.0,
     'in_gxr': 25.0, 'in_Simg': 16.0, 'in_dbc': 16.0, 'in_dWc': 16.0, 'heads_Y': 42.0, 'heads_dX': 27.0, 'heads_tot': 16.0}
# Worst ratio error / (U cond) seen on an MI355X (gfx950), by output (test_mlp_ends_fp64_gpu.py::test_worst_ratios prints a
# run's).  A record, not a bound: no K above is derived from it.
GPU_SEEN = {'rowdot': 0.484, 'seg_sum': 3.503, 'coldot': 3.822, 'outer_mask': 2.749, 'act_bwd': 1.421, 'dec_l0': 1.349,
            'latent_bias': 1.697, 'dWl': 2.265, 'dz': 1.730, 'fourier_fwd': 3.867, 'fourier_bwd': 2.16, 'out_D': 2.701,
            'out_tot': 0.326, 'in_gxr': 2.065, 'in_Simg': 1.070, 'in_dbc': 0.148, 'in_dWc': 0.325, 'heads_Y': 6.392,
            'heads_dX': 3.319, 'heads_tot': 0.321}
# tvae_fourier_bwd next to FOURIER_SIN_ABS: 2.16 above is its error WITHOUT the floor, and the floor was not drawn on in any
# case -- (error - K U cond) / floor stayed below -0.61.  With |b| up to 2 pi in A, K U cond alone allows about 16 U 2 pi =
# 6e-6 per term, more than the floor adds; the floor is kept as the existing test states it, not tightened.
FOURIER_SIN_SEEN = {'worst (error - K U cond) / floor': -0.611, 'worst error without the floor, in U cond': 2.16}

ONE_M = 1.0 - 2.0 ** -24      # the fp32 number below 1
SPECIALS = [0.0, -0.0, 1e-30, -1e-30, ONE_M, -ONE_M]


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _v(t, dt, cond):
    return t.double().abs() if cond else t.to(dt)


def ratio(got, ref, cond, floor=None):
    """Worst |got - ref| / (U cond) over ALL elements; an absolute `floor` is taken off the error first.  Where cond is zero the
    result has to be exact; a non-finite result gives inf."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    if floor is not None:
        err = (err - floor).clamp_min(0.0)
    r = torch.where(cond > 0, err / (U * cond.clamp_min(1e-300)), torch.where(err > 0, math.inf, 0.0).double())
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return float(r.max())


def ratios(got, ref, cond, floor=None):
    """The same for dicts of outputs: name -> worst ratio."""
    return {n_: ratio(got[n_], ref[n_], cond[n_], (floor or {}).get(n_)) for n_ in ref}


def both(fn, *args):
    """(reference, condition quantity) of an operation below."""
    return fn(*args, dt=F64, cond=False), fn(*args, dt=F64, cond=True)


# ---- activations ------------------------------------------------------------------------------------------------------------
def dact(y, act, dt=F64, cond=False):
    """act'(.) from the stored output y; cond=True: its condition quantity."""
    y = y.double() if cond else y.to(dt)
    if act == 1:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))
    if act == 2:
        return 1 + y * y if cond else 1 - y * y
    return torch.ones_like(y)


def act_apply(x, act):
    return x if act == 0 else (F_.leaky_relu(x, SLOPE) if act == 1 else torch.tanh(x))


def stored_output(rows, N, act, seed, panel):
    """A [rows][N] fp32 activation output (tanh: inside +-1) with SPECIALS planted at plant_columns()."""
    H = act_apply(rnd(rows, N, seed=seed), act).contiguous()
    for k_, c in enumerate(plant_columns(N, panel)):
        for r in range(rows):
            H[r, c] = SPECIALS[(r + k_) % len(SPECIALS)]
    return H


def plant_columns(N, panel):
    """First and last column of every panel, the columns around the last panel boundary, the first and the last valid column of
    the last (ragged) float4 and the column before it."""
    cols = {0, 1, N - 1, N - 2, 4 * ((N - 1) // 4), 4 * ((N - 1) // 4) - 1}
    for p in range(panel, N, panel):
        cols |= {p - 1, p}
    return sorted(c for c in cols if 0 <= c < N)


# ---- the operations ---------------------------------------------------------------------------------------------------------
def rowdot_seg(X, V, seglen, dt=F64, cond=False):
    """X [M][N], V [N][no] or None -> out [nseg][M][no]"""
    X = _v(X, dt, cond)
    N = X.shape[1]
    segs = [slice(s, min(N, s + seglen)) for s in range(0, N, seglen)]
    if V is None:
        return torch.stack([X[:, s].sum(1, keepdim=True) for s in segs])
    V = _v(V, dt, cond)
    return torch.stack([X[:, s] @ V[s] for s in segs])


def seg_sum(X, out0, scale, accumulate, dt=F64, cond=False):
    """X [S][L], out0 [L] -> out0 * accumulate + scale * sum_s X"""
    s = _v(X, dt, cond).sum(0) * (abs(scale) if cond else scale)
    return s + _v(out0, dt, cond) if accumulate else s


def coldot(X, W, b, dt=F64, cond=False):
    """X [M][N], W [no][M], b [no] or None -> out [N][no]"""
    out = (_v(W, dt, cond) @ _v(X, dt, cond)).t()
    return out if b is None else out + _v(b, dt, cond)


def outer_mask(dy, W, H, act, dt=F64, cond=False):
    """dy [N][no], W [no][M], H [M][N] -> D [M][N]"""
    return (_v(W, dt, cond).t() @ _v(dy, dt, cond).t()) * dact(H, act, dt, cond)


def act_bwd(dY, Y, act, dt=F64, cond=False):
    return _v(dY, dt, cond) * dact(Y, act, dt, cond)


def dec_l0_fwd(xr, Wc, bc, LB, Np, act, dt=F64, cond=False):
    """xr [Nt][2], Wc [F][2], bc [F], LB [B][F] or None -> h [F][Nt]"""
    def pre(dt_, c_):
        p = _v(xr, dt_, c_) @ _v(Wc, dt_, c_).t() + _v(bc, dt_, c_)
        return p if LB is None else p + _v(LB, dt_, c_).repeat_interleave(Np, 0)
    if not cond:
        return act_apply(pre(dt, False), act).t()
    p, c = pre(F64, False), pre(F64, True)
    if act == 1:
        lip = torch.where(p < -64 * U * c, torch.full_like(p, SLOPE), torch.ones_like(p))
    else:
        lip = 1 - torch.tanh(p) ** 2 if act == 2 else torch.ones_like(p)
    return (act_apply(p, act).abs() + c * lip).t()


def latent_bias(Wl, z, dt=F64, cond=False):
    """Wl [F][zd], z [B][zd] -> LB [B][F]"""
    return _v(z, dt, cond) @ _v(Wl, dt, cond).t()


def latent_bwd(S, Wl, z, dt=F64, cond=False):
    """S [B][F] -> {dWl [F][zd], dz [B][zd]}"""
    S = _v(S, dt, cond)
    return {'dWl': S.t() @ _v(z, dt, cond), 'dz': S @ _v(Wl, dt, cond)}


def fourier_arg(xr, Wf, bf, sigma):
    """-> w [F][2] fp32, the fp32-rounded argument [Nt][F], A = |x0 w0| + |x1 w1| + |b| [Nt][F] float64"""
    w = Wf / torch.tensor(sigma, dtype=F32)
    t0, t1 = xr[:, 0:1] * w[:, 0][None, :], xr[:, 1:2] * w[:, 1][None, :]
    return w, t0 + t1 + bf[None, :], t0.double().abs() + t1.double().abs() + bf.double().abs()[None, :]


def fourier_fwd(xr, Wf, bf, sigma, dt=F64, cond=False):
    """-> feat [F][Nt]"""
    w, a, A = fourier_arg(xr, Wf, bf, sigma)
    if cond:
        return (torch.cos(a.double()).abs() + A * torch.sin(a.double()).abs()).t()
    return torch.cos(a.to(dt)).t()


def fourier_bwd(xr, Wf, bf, sigma, g, dt=F64, cond=False):
    """g [F][Nt] -> gxr [Nt][2]"""
    w, a, A = fourier_arg(xr, Wf, bf, sigma)
    if cond:
        a = a.double()
        return ((torch.sin(a).abs() + A * torch.cos(a).abs()) * g.double().abs().t()) @ w.double().abs()
    return (-torch.sin(a.to(dt)) * g.to(dt).t()) @ w.to(dt)


def fourier_bwd_floor(xr, Wf, bf, sigma, g):
    w = fourier_arg(xr, Wf, bf, sigma)[0]
    return FOURIER_SIN_ABS * (g.double().abs().t() @ w.double().abs())


def dec_out_bwd(gy, Wo, H, act, dt=F64, cond=False):
    """gy [N][no], Wo [no][F], H [F][N] -> {out_D [F][N], out_tot [1 + no][F]}"""
    gy_, H_ = _v(gy, dt, cond), _v(H, dt, cond)
    D = (_v(Wo, dt, cond).t() @ gy_.t()) * dact(H, act, dt, cond)
    return {'out_D': D, 'out_tot': torch.cat([D.sum(1)[None], (H_ @ gy_).t()])}


def dec_in_bwd(d, xr, Wc, B, Np, dt=F64, cond=False):
    """d [F][B Np], xr [B Np][2], Wc [F][2] -> gxr [B Np][2], Simg [B][F], dbc [F], dWc [F][2]"""
    d = _v(d, dt, cond)
    return {'in_gxr': d.t() @ _v(Wc, dt, cond), 'in_Simg': d.view(d.shape[0], B, Np).sum(2).t(), 'in_dbc': d.sum(1),
            'in_dWc': d @ _v(xr, dt, cond)}


def heads_fwd(W, X, b, dt=F64, cond=False):
    """W [nh][C], X [C][N], b [nh] or None -> Y [nh][N]"""
    Y = _v(W, dt, cond) @ _v(X, dt, cond)
    return Y if b is None else Y + _v(b, dt, cond)[:, None]


def heads_bwd(W, dY, X, act, dt=F64, cond=False):
    """-> {heads_dX [C][N], heads_tot [nh + 1][C]}"""
    dY_ = _v(dY, dt, cond)
    dX = (_v(W, dt, cond).t() @ dY_) * dact(X, act, dt, cond)
    return {'heads_dX': dX, 'heads_tot': torch.cat([dY_ @ _v(X, dt, cond).t(), dX.sum(1)[None]])}


# ---- cases ------------------------------------------------------------------------------------------------------------------
def ld_pad4(N):
    return (N + 3) // 4 * 4 + 4


# tvae_rowdot_seg without V, M = 5: (seglen, N).  300: n4 = 75, a trailing float4 only and idle threads, ragged last segment of 123
# (tail 3); 250 < 300: one short segment; 1600: n4 = 400, threads 0-143 pair up, the rest take the trailing float4, last segment
# 1001 (tail 1); 3151: a second paired trip (threads 0-18), the trailing float4 (19-255) and a dword tail of 3 -- segments 1, 2, 3
# begin at 3151, 6302, 9453 (not multiples of 4): the dword form; segment 4 begins at 12604: the 16-byte form again, ragged (777).
ROWSUM_SHAPES = [(300, 723), (300, 250), (1600, 2601), (3151, 13381)]
ROWSUM_LAYOUTS = ['aligned', 'view', 'ldx1']     # ldx = ld_pad4(N), X 16-byte aligned | the same, X one float further | ldx = 4k + 1
ROWSUM_CASES = list(itertools.product(ROWSUM_SHAPES, ROWSUM_LAYOUTS))
ROWSUM_M = 5
ROWDOT_V_CASES = [1, 2, 3, 4]                    # no; M = 37, N = 1203, seglen = 500
# amax: (row, column) of the planted -77.5 in the (3151, 13381) case, by the load that meets it
AMAX_PLANTS = {'paired-first': (2, 100), 'paired-second': (2, 4 * (256 + 10)), 'paired-trip2': (1, 4 * (512 + 7)),
               'trailing-float4': (3, 4 * 600), 'dword-tail': (4, 3149), 'dword-form-segment': (0, 3151 + 50),
               'ragged-last-segment': (2, 12604 + 775)}


@functools.lru_cache(maxsize=None)
def rowsum_case(seglen, N):
    return rnd(ROWSUM_M, N, seed=seglen + N)


@functools.lru_cache(maxsize=None)
def rowsum_ref(seglen, N):
    return both(rowdot_seg, rowsum_case(seglen, N), None, seglen)


@functools.lru_cache(maxsize=None)
def rowdot_v_case(no):
    return rnd(37, 1203, seed=10 + no), rnd(1203, no, seed=20 + no)


# tvae_seg_sum: both sides of wave | tile | plain thresholds, and the tile kernel's leftover loop
SEG_SUM_CASES = [(32, 64), (31, 64), (64, 65), (63, 65), (64, 65536), (64, 65537), (67, 65), (113, 130)]
SEG_SUM_MODES = [(0.25, 1), (1.0, 0)]            # (scale, accumulate)


@functools.lru_cache(maxsize=None)
def seg_sum_case(S, L):
    return rnd(S, L, seed=S + L), rnd(L, seed=S * L)


# tvae_coldot / tvae_outer_mask / tvae_act_bwd: (no, layout, act, bias); layout 0: W [no][M] (wsm, wso) = (1, M); 1: W [M][no] (no, 1)
SKINNY_M, SKINNY_N = 70, 300
SKINNY_CASES = [(no, lay, (no + lay) % 3, no % 2 == 1) for no in (1, 2, 3, 4) for lay in (0, 1)]


@functools.lru_cache(maxsize=None)
def skinny_case(no, act):
    """-> X = H [M][N] (a stored output with planted values), W [no][M], b [no], dy [N][no]"""
    M, N = SKINNY_M, SKINNY_N
    return stored_output(M, N, act, 30 + no, 256), rnd(no, M, seed=31 + no), rnd(no, seed=32 + no), rnd(N, no, seed=33 + no)


# tvae_dec_l0_fwd / tvae_latent_bias: (F, zd, act, LB given); B = 3, Np = 100 (an image boundary inside the second workgroup)
L0_B, L0_NP = 3, 100
L0_CASES = [(5, 1, 1, True), (16, 2, 2, True), (37, 5, 0, True), (37, 2, 1, False), (5, 5, 2, True), (16, 1, 0, False)]
LATENT_BWD_CASES = [(7, 65, 3), (65, 7, 5), (129, 300, 2)]      # (B, F, zd)


@functools.lru_cache(maxsize=None)
def l0_case(F, zd):
    """-> xr [Nt][2], Wc, bc, Wl [F][zd], z [B][zd]"""
    Nt = L0_B * L0_NP
    xr = torch.rand(Nt, 2, generator=torch.Generator().manual_seed(40 + F)) * 2 - 1
    return xr, rnd(F, 2, seed=41 + F), rnd(F, seed=42 + F), rnd(F, zd, seed=43 + F + zd), rnd(L0_B, zd, seed=44 + zd)


@functools.lru_cache(maxsize=None)
def latent_bwd_case(B, F, zd):
    return rnd(B, F, seed=50 + B), rnd(F, zd, seed=51 + F), rnd(B, zd, seed=52 + B)


# tvae_fourier_fwd / _bwd: Nt = 300 (a ragged second workgroup), coordinates in +-1.5
FOURIER_NT = 300
FOURIER_SIGMAS = [2.0 / 27, 0.01]
FOURIER_FWD_CASES = list(itertools.product([5, 48, 300], FOURIER_SIGMAS))
FOURIER_BWD_CASES = list(itertools.product([5, 256, 257, 300, 1024], FOURIER_SIGMAS))


@functools.lru_cache(maxsize=None)
def fourier_case(F):
    """-> xr [Nt][2], Wf [F][2], bf [F], g [F][Nt]"""
    xr = (torch.rand(FOURIER_NT, 2, generator=torch.Generator().manual_seed(60 + F)) * 2 - 1) * 1.5
    bf = torch.rand(F, generator=torch.Generator().manual_seed(61 + F)) * 2 * math.pi
    return xr, rnd(F, 2, seed=62 + F), bf, rnd(F, FOURIER_NT, seed=63 + F)


# tvae_dec_out_bwd: (F, N, ldh, ldd, n_out, act).  fs = 8 row slices | vec = 0 | vec = 1 with the element-wise tail of load4 /
# store4 | F < 16 and a one-column second panel
DEC_OUT_CASES = [(130, 1000, 1000, 1000, 3, 2), (37, 1027, 1027, 1027, 2, 1), (37, 2051, 2052, 2056, 4, 2), (5, 1025, 1028, 1028, 1, 0)]


@functools.lru_cache(maxsize=None)
def dec_out_case(F, N, no, act):
    """-> gy [N][no], Wo [no][F], H [F][N]"""
    return rnd(N, no, seed=70 + N), rnd(no, F, seed=71 + F), stored_output(F, N, act, 72 + N, 1024)


@functools.lru_cache(maxsize=None)
def dec_out_ref(F, N, no, act):
    return both(dec_out_bwd, *dec_out_case(F, N, no, act), act)


# tvae_dec_in_bwd: (F, B, Np, ldd).  padded stride | vec = 0, two panels per image | vec = 1, a four-column second panel | more
# than the 64 images of one round of the totals
DEC_IN_CASES = [(5, 3, 100, 304), (33, 2, 1089, 2178), (8, 2, 1028, 2056), (64, 70, 36, 2520)]


@functools.lru_cache(maxsize=None)
def dec_in_case(F, B, Np):
    """-> d [F][B Np], xr [B Np][2], Wc [F][2]"""
    return rnd(F, B * Np, seed=80 + F), rnd(B * Np, 2, seed=81 + B), rnd(F, 2, seed=82 + F)


# tvae_heads_fwd / _bwd: (nh, C, (N, ldx, ldy = lddx), act, bias given): every instance at every layout
HEADS_LAYOUTS = [(1001, 1001, 1001), (1001, 1004, 1008), (1024, 1024, 1024)]
HEADS_CASES = [(nh, (5, 33)[(nh + i) % 2], lay, (nh + i) % 3, (nh + i) % 4 != 0)
               for nh in range(1, 9) for i, lay in enumerate(HEADS_LAYOUTS)]
HEADS_BIG = (3, 8, 256 * 512 - 37, 1)            # nh, C, N, act: 256 panels, the two-stage totals when the workspace has room


@functools.lru_cache(maxsize=None)
def heads_case(nh, C, N, act):
    """-> W [nh][C], b [nh], X [C][N] (a stored output with planted values), dY [nh][N]"""
    return rnd(nh, C, seed=90 + nh, scale=C ** -0.5), rnd(nh, seed=91 + nh), stored_output(C, N, act, 92 + N + C, 512), rnd(nh, N, seed=93 + N)


@functools.lru_cache(maxsize=8)
def heads_ref(nh, C, N, act):
    W, b, X, dY = heads_case(nh, C, N, act)
    return both(heads_bwd, W, dY, X, act)
