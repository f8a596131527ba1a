"""float64 restatement of the rotated filter bank (tvae_rotate_bank_fwd / _bwd) as ONE sparse operator built from the dense tap
table tvae.tables.rotation_taps(k, R) -- never from the CSR form the backward kernel walks: the backward reference is the
transpose of the forward operator, so tables.rotation_taps_csr is under test too.  A plain helper module (test_bank_ref_cpu.py,
test_rotate_bank_fp64_gpu.py).

    bank[c R + r][ci k^2 + d] = sum_t w[r][d][t] weight[c][ci][idx[r][d][t]]          A [R k^2][k^2], 4 entries per row at most

Bounds (u = 2^-24; sums of products in fp32, no measurement needed): an n-term sum of products evaluated in any order is within
n u / (1 - n u) < (n + 1) u of the exact one, times sum |w_t x_t|.  n = 4 in the forward; in the backward n is the number of
taps that read the source pixel (its list length), and `accumulate` adds one more term, the initial dweight."""
import numpy as np
import torch

U = 2.0 ** -24


def operator(k, R):
    """-> (A, absA sparse float64 [R k^2][k^2], n [k^2]: entries per column, int64)."""
    from tvae import tables
    idx, wgt = tables.rotation_taps(k, R)
    k2 = k * k
    r_i, d_i, t_i = np.nonzero((idx >= 0) & (wgt != 0))
    rows = torch.from_numpy((r_i * k2 + d_i).astype(np.int64))
    cols = torch.from_numpy(idx[r_i, d_i, t_i].astype(np.int64))
    vals = torch.from_numpy(wgt[r_i, d_i, t_i].astype(np.float64))
    ij = torch.stack([rows, cols])
    A = torch.sparse_coo_tensor(ij, vals, (R * k2, k2)).coalesce()
    absA = torch.sparse_coo_tensor(ij, vals.abs(), (R * k2, k2)).coalesce()
    n = torch.bincount(cols, minlength=k2)
    return A, absA, n


def forward(weight, k, R):
    """weight (C, Cin, 1, k, k) fp32 -> (bank [C R][Cin k^2] float64, cond = sum |w x| of every element)."""
    C, Cin = weight.shape[:2]
    A, absA, _ = operator(k, R)
    W = weight.double().reshape(C * Cin, k * k)

    def ap(M, X):
        return torch.sparse.mm(M, X.t()).t().reshape(C, Cin, R, k * k).permute(0, 2, 1, 3).reshape(C * R, Cin * k * k)
    return ap(A, W), ap(absA, W.abs())


def backward(dbank, C, Cin, k, R, init=None):
    """dbank [C R][Cin k^2] fp32 -> (dweight [C Cin][k^2] float64, cond, n [k^2]); init: the initial dweight of accumulate = 1."""
    A, absA, n = operator(k, R)
    G = dbank.double().reshape(C, R, Cin, k * k).permute(0, 2, 1, 3).reshape(C * Cin, R * k * k)
    dW = torch.sparse.mm(A.t(), G.t()).t()
    cond = torch.sparse.mm(absA.t(), G.abs().t()).t()
    if init is not None:
        dW = dW + init.double().reshape(C * Cin, k * k)
        cond = cond + init.double().abs().reshape(C * Cin, k * k)
        n = n + 1
    return dW, cond, n
