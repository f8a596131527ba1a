"""Plain-torch float64 restatement of the attention head (tvae.ops.HeadFn: csrc/small_kernels.hpp, attn_head_*), a helper
module used by test_head_ref_cpu.py, test_head_fp64_gpu.py and test_midsize_kernels.py.

It takes the four tables as DATA -- the fp32 values the device is given, cast to double -- so it serves any (R, P), square grid
or not.  Everything is differentiable by autograd.  There is no dead-position special case: in double exp(q) does not
underflow at the logits the tests use (q > -700), and a position whose fp32 expf(q) is 0 contributes less than 1e-80 here.

    l_j  = heads[0][j] + p_r[r]                      attn
    q_j  = l_j - logsumexp(l)                        q
    d_j  = l_j - log E_j,   a = softmax(d)           a      (Gumbel-softmax with Exp(1) draws)
    theta = sum_j a_j tmu_j + eps_t sum_j a_j tsd_j,   tmu = heads[1] + theta_off_scale off[r],  tsd = exp(heads[2]) + 1e-6
    z_c   = sum_j a_j zmu_cj + eps_z[c] sum_j a_j zsd_cj
    dx    = sum_j a_j grid[hw]
    kl    = sum_j exp(q_j) (q_j - p_tr_j + KLt_j + sum_c KLz_cj)
    KLt = (vr + ((tmu - off[r]) / sigma_p)^2 - 1 - log vr) / 2, vr = (tsd / sigma_p)^2;   KLz = (sd^2 + mu^2 - 1 - log sd^2) / 2

CONDITION QUANTITIES (head(): second return value; block_conditions()).  u = 2^-24.  An fp32 evaluation rounds every
intermediate; what a rounding of relative size u does to an output is bounded by u times the quantities below.
  attn_j : |heads0_j| + |p_r|                                           (one add)
  q_j    : cq_j = 1 + |l_j| + 2 |m1| + |lse| + sum_i exp(q_i) |l_i|     (l - lse; lse = m1 + log sum exp(l - m1): the argument of
           every exponential carries u (|l_i| + |m1|), the sum weighs those by exp(q_i))
  a_j    : ca_j = 1 + k_j + sum_i a_i k_i,  k_j = 1 + |l_j| + |log E_j| + |d_j| + 2 |m2|      (relative: an absolute error of the
           exponent d_j - m2 is a relative error of a_j; the normaliser carries the a-weighted mean of the k_i)
  z, theta, dx : sum_j |term_j| ca_j, term_j the summand (a_j |mu_j| + |eps| a_j sd_j, a_j |grid|)
  kl     : sum_j exp(q_j) (1 + cq_j) (|q_j| + |p_tr_j| + sum of the absolute values of the addends of KLt and KLz)
  dheads block (row, image): max-norm relative to the block's own maximum.  Rows >= 1 are a_j g + gkl exp(q_j) (...): an error
           at position j relative to the block maximum is at most (a_j / max a) ca_j resp. (exp(q_j) / max exp(q)) (1 + cq_j);
           cb = 1 + max_j (a_j / max a) ca_j + max_j (exp(q_j) / max exp(q)) (1 + cq_j).
           Row 0 is dl_j = a_j (da_j - sa) + dq_j - exp(q_j) sq + g_attn_j with sa = sum_i a_i da_i, sq = sum_i dq_i and
           dq_j = dqo_j + g_q_j (dqo_j = gkl exp(q_j) (...), relative error 1 + cq_j; g_q_j exact) -- two cancelling differences.
           First order, per position:
             e_j = a_j ca_j |da_j| + a_j (ca_j |sa| + Sa) + D_j + exp(q_j) ((1 + cq_j) |sq| + Sq) + |g_attn_j|,
             D_j = |dqo_j| (1 + cq_j) + |g_q_j|,   Sa = sum_i a_i ca_i |da_i|,   Sq = sum_i D_i
           and the block's condition is max_j e_j / max_j |dl_j| (not below 1).
The constants K of the bounds K u (condition) are measured by test_head_ref_cpu.py (fp32 on the CPU against this file) and kept
in K below: 8 x the worst measured ratio, not below 16."""
import math

import torch

U = 2.0 ** -24
EPS_STD = float(torch.tensor(1e-6, dtype=torch.float32))
NAMES = ['attn', 'q', 'a', 'z', 'theta', 'dx', 'kl']

# K per checked quantity: max(16, 8 x worst ratio |fp32 CPU oracle - head_ref| / (u condition)) over the cases of
# test_head_ref_cpu.py::test_budget_constants, which prints the ratios and asserts that these constants cover them.
#          attn  q     a     z     theta dx    kl    dheads
# ratio    1.00  1.00  0.47  0.09  0.75  0.17  0.19  0.17
K = {'attn': 16.0, 'q': 16.0, 'a': 16.0, 'z': 16.0, 'theta': 16.0, 'dx': 16.0, 'kl': 16.0, 'dheads': 16.0}


def case_inputs(RP, zd, peaked=False):
    """The inputs of test_midsize_kernels._inputs (B = 3: E at 1e-30 and 1 - 2^-24, image 1 shifted by -200, every other logit of
    image 2 shifted by -200); peaked: the logits x 30 instead of x 4 UNDER the same shifts (a near one-hot softmax)."""
    from test_midsize_kernels import _inputs
    hd, E, eps_z, eps_t = _inputs(RP, zd)
    if peaked:
        S = torch.zeros(3 * RP)
        S[RP:2 * RP] = 200.0
        S[2 * RP + 1:3 * RP:2] = 200.0
        hd[0] = (hd[0] + S) * 7.5 - S
    return hd, E, eps_z, eps_t


def upstream(B, RP, zd, seven):
    """Upstream gradients at coefficient 1: all seven, or only the four the training step has (z, theta, dx, kl)."""
    shapes = [(B, RP)] * 3 + [(B, zd), (B,), (B, 2), (B,)]
    ups = [torch.randn(*s, generator=torch.Generator().manual_seed(20 + i)) for i, s in enumerate(shapes)]
    if not seven:
        ups[0] = ups[1] = ups[2] = None
    return ups


def tables_f64(tb):
    """(p_r, off, grid, p_tr, sigma_p, theta_off_scale) of a tvae.ops.HeadTables-like object, the device's fp32 values as
    double on the CPU (sigma_p rounded to fp32 as the C ABI takes it)."""
    return (tb.p_r.detach().double().cpu(), tb.off.detach().double().cpu(), tb.grid.detach().double().cpu(),
            tb.p_tr.detach().double().cpu(), float(torch.tensor(tb.sigma_p, dtype=torch.float32)), float(tb.theta_off_scale))


def head(heads, E, eps_z, eps_t, p_r, off, grid, p_tr, sigma_p, theta_off_scale):
    """heads [3 + 2 zd][B][RP] (double, may require grad), E [B][RP], eps_z [B][zd], eps_t [B]; tables as tables_f64 gives them.
    -> (outs, cond, mid): outs = (attn, q, a [B][RP], z [B][zd], theta [B], dx [B][2], kl [B]); cond: name -> condition
    quantity shaped like the output (no gradient); mid: the intermediates block_conditions() needs."""
    nh, B, RP = heads.shape
    zd = (nh - 3) // 2
    R, P = p_r.numel(), grid.shape[0]
    assert nh == 3 + 2 * zd and RP == R * P and p_tr.numel() == RP
    E, eps_z, eps_t = E.double(), eps_z.double().view(B, zd), eps_t.double().view(B)
    pr_j = p_r.repeat_interleave(P)
    off_j = off.repeat_interleave(P)
    g_j = grid.repeat(R, 1)                                                  # [RP][2]
    l = heads[0] + pr_j
    m1 = l.detach().max(1, keepdim=True).values
    lse = m1 + torch.log(torch.exp(l - m1).sum(1, keepdim=True))
    q = l - lse
    logE = torch.log(E)
    d = l - logE
    m2 = d.detach().max(1, keepdim=True).values
    e2 = torch.exp(d - m2)
    a = e2 / e2.sum(1, keepdim=True)
    eq = torch.exp(q)
    tmu = heads[1] + theta_off_scale * off_j
    tsd = torch.exp(heads[2]) + EPS_STD
    theta = (a * tmu).sum(1) + eps_t * (a * tsd).sum(1)
    zmu, zsd = heads[3:3 + zd], torch.exp(heads[3 + zd:]) + EPS_STD           # [zd][B][RP]
    z = ((a * zmu).sum(2) + eps_z.t() * (a * zsd).sum(2)).t()
    dx = a @ g_j
    vr = (tsd / sigma_p) ** 2
    t1 = ((tmu - off_j) / sigma_p) ** 2
    klt = 0.5 * (vr + t1 - 1.0 - torch.log(vr))
    klz = (0.5 * (zsd ** 2 + zmu ** 2 - 1.0 - torch.log(zsd ** 2))).sum(0)
    kl = (eq * (q - p_tr + klt + klz)).sum(1)
    outs = (l, q, a, z, theta, dx, kl)
    with torch.no_grad():
        cq = 1.0 + l.abs() + 2.0 * m1.abs() + lse.abs() + (eq * l.abs()).sum(1, keepdim=True)
        k = 1.0 + l.abs() + logE.abs() + d.abs() + 2.0 * m2.abs()
        ca = 1.0 + k + (a * k).sum(1, keepdim=True)
        aw = a * ca
        klabs = 0.5 * (vr + t1 + 1.0 + torch.log(vr).abs()) + \
            (0.5 * (zsd ** 2 + zmu ** 2 + 1.0 + torch.log(zsd ** 2).abs())).sum(0)
        cond = {
            'attn': heads[0].abs() + pr_j.abs(),
            'q': cq,
            'a': ca,
            'z': ((aw * zmu.abs()).sum(2) + eps_z.t().abs() * (aw * zsd).sum(2)).t(),
            'theta': (aw * tmu.abs()).sum(1) + eps_t.abs() * (aw * tsd).sum(1),
            'dx': aw @ g_j.abs(),
            'kl': (eq * (1.0 + cq) * (q.abs() + p_tr.abs() + klabs)).sum(1),
        }
        cond = {n_: c.detach() for n_, c in cond.items()}
    return outs, cond, dict(a=a, q=q, ca=ca, cq=cq)


def head_with_grad(heads, E, eps_z, eps_t, tabs, ups):
    """Forward and autograd backward of sum_i <out_i, ups_i> (ups: seven upstream gradients, None where absent).
    heads [3 + 2 zd][B][RP] double.  -> (outs detached, cond, dheads [nh][B][RP], cblock [nh][B]): cblock the condition quantity
    of every (head row, image) block of dheads (module docstring)."""
    hr = heads.detach().clone().double().requires_grad_(True)
    outs, cond, mid = head(hr, E, eps_z, eps_t, *tabs)
    loss = sum((o * u_.double().view_as(o)).sum() for o, u_ in zip(outs, ups) if u_ is not None)
    dh, da, dq = torch.autograd.grad(loss, [hr, mid['a'], mid['q']])
    with torch.no_grad():
        a, eq = mid['a'].detach(), torch.exp(mid['q'].detach())
        cb = 1.0 + (a / a.max(1, keepdim=True).values * mid['ca']).max(1).values + \
            (eq / eq.max(1, keepdim=True).values * (1.0 + mid['cq'])).max(1).values                      # [B]
        ca, cq1 = mid['ca'], 1.0 + mid['cq']
        g_attn, g_q = (torch.zeros_like(a) if u_ is None else u_.double().view_as(a) for u_ in ups[:2])
        dqo = (dq - g_q).abs() * cq1 + g_q.abs()
        sa, sq = (a * da).sum(1, keepdim=True).abs(), dq.sum(1, keepdim=True).abs()
        Sa, Sq = (a * ca * da.abs()).sum(1, keepdim=True), dqo.sum(1, keepdim=True)
        e0 = a * ca * da.abs() + a * (ca * sa + Sa) + dqo + eq * (cq1 * sq + Sq) + g_attn.abs()
        den = dh[0].abs().max(1).values
        c0 = torch.where(den > 0, e0.max(1).values / den.clamp_min(1e-300), torch.ones_like(den)).clamp_min(1.0)
        cblock = cb.expand(hr.shape[0], -1).clone()
        cblock[0] = c0
    return [o.detach() for o in outs], cond, dh, cblock


def ratios(got, dh_got, outs, cond, dh, cblock):
    """Worst ratio error / (u condition) per checked quantity: got (seven outputs) and dh_got against head_with_grad()'s results.
    attn, q absolute per element; a relative per element where the reference is >= 2^-100 (below: |got| <= 2^-99 is asserted
    here, nothing is skipped); z, theta, dx, kl per image and component; dheads per (row, image) block, max-norm relative to the
    block's own reference maximum."""
    r = {}
    g64 = [torch.as_tensor(g_).detach().double().cpu().view_as(o) for g_, o in zip(got, outs)]
    for i, n_ in enumerate(NAMES):
        err = (g64[i] - outs[i]).abs()
        if n_ == 'a':
            big = outs[i] >= 2.0 ** -100
            assert bool((g64[i][~big].abs() <= 2.0 ** -99).all()), 'a: a value above 2^-99 where the reference is below 2^-100'
            err = torch.where(big, err / outs[i].clamp_min(2.0 ** -100), torch.zeros_like(err))
        r[n_] = float((err / (U * cond[n_])).max())
    dg = torch.as_tensor(dh_got).detach().double().cpu().view_as(dh)
    bmax = dh.abs().amax(2)
    berr = (dg - dh).abs().amax(2)
    rel = torch.where(bmax > 0, berr / bmax.clamp_min(1e-300), berr)           # an all-zero block has to be all zero
    r['dheads'] = float((rel / (U * cblock)).max())
    r['dheads_blocks'] = rel / (U * cblock)
    return r


def assert_within(r, what=''):
    for n_, k_ in K.items():
        assert math.isfinite(r[n_]) and r[n_] <= k_, (what, n_, r[n_], k_)
