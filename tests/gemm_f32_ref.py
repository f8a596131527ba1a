"""float64 restatements of the exact-fp32 entry points -- tvae_linear_fwd / _dgrad / _wgrad (csrc/abi_linear_f32.hip) and
tvae_conv1_fwd / _wgrad (csrc/abi_conv_f32.hip) -- with the condition quantities of their error bound, the planted values and the
case lists that test_gemm_f32_ref_cpu.py (routes, K, mutations: CPU) and test_gemm_f32_fp64_gpu.py (the kernels) both run.
A plain helper module; it works on whatever device its arguments live on.

Every operation is ONE expression in the dtype `dt`: float64 is the reference, cond=True evaluates the same expression on the
absolute values of its operands -- the per-element CONDITION QUANTITY, the sum of the absolute values of the terms added.

    fwd         Y  = act(W X + b + gbias[n // group] + res)      cond = |W| |X| + |b| + |gbias| + |res|  (of the PRE-activation)
    dgrad       dX = act'(aux) . (W^T d + add)                   cond = |act'|(aux) . (|W^T| |d| + |add|)
                     act'(a): lrelu  a > 0 ? 1 : slope  (+0.0 and -0.0 are not positive);  tanh  1 - a a  (cond: 1 + a a)
    wgrad       dW = d X^T (+ init)                              cond = |d| |X^T| (+ |init|)
    conv fwd    out[c][b][r][p] = act(sum_k bank[c R + r][k] patch(b, k, p) + bias[c])     in the [C][B][R][Ho Ho] layout
    conv wgrad  dbank[c R + r][k] = sum_{b, p} dpre[c][b][r][p] patch(b, k, p)             (conv2d_weight)

patch(b, k = (ci, u, v), p = (h, w)) = ypad[b][ci][h + u][w + v] is an explicit unfold of the zero-padded image (checked once
against F.conv2d / torch.nn.grad.conv2d_weight in float64 by the CPU file).  The activations are 1-Lipschitz, so the error of the
pre-activation carries over at most 1 : 1 and a pre-activation within rounding of 0 is compared like any other; tanhf's own
error (a few ulp of |tanh| <= |pre| <= cond) lies inside K >= 16.

A kernel result `got` has to satisfy, in EVERY element,

    |got - ref| <= K[name] * 2^-24 * cond + TINY,         exactly where cond == 0.

No element, row or case is exempt.  TINY = 2^-119 (products that underflow fp32's normal range, 2^-149 each, tens of thousands).

K: never from the kernels.  CPU arithmetic (the same expressions with dt = float32) against this file on every case below
(test_gemm_f32_ref_cpu.py::test_budget_constants measures and prints them, on one thread); K = max(16, 8 x worst ratio) per
output:

    output       ratio     8 x     K
    fwd           3.678   29.42    30
    dgrad         4.896   39.17    40
    wgrad         1.696   13.57    16
    conv_fwd      4.315   34.52    35
    conv_wgrad    1.712   13.70    16

Strided tensors: pad columns of inputs hold PAD_IN (a read of one shows in the result), outputs start as NaN in their columns and
SENTINEL in their pad columns, which must come back holding it; an element nobody writes fails.

Planted values (what a wrong kernel cannot hide behind a long condition sum): rows 0, 1, 2 of the A operand (weight / bank / dY /
dpre row) have exactly ONE non-zero entry, at the first reduction index, the last, and the last before a 16-step boundary; row 3
is scaled by 2^-20 (errors are per element, so a wrong small row shows); aux holds +0.0, -0.0, 1e-30, -1e-30 at the tile corners
(rows 0, 63, 64, 127 x columns 0, 31, 32, 127); the last row of the forward cases with a residual has res = -fp32(W X + b + gbias),
so its pre-activations lie within rounding of 0.
"""
import math

import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
SLOPE = float(torch.tensor(0.01, dtype=F32))                  # what the kernels get: fp32(0.01)
UNIT = 2.0 ** -24
TINY = 2.0 ** -119
SENTINEL = -7777.0            # prefill of strided outputs: pad columns must come back holding it
PAD_IN = 1e30                 # pad columns of strided inputs: a read of one shows in the result
BM = BN = 128
BK = 16

K = {'fwd': 30.0, 'dgrad': 40.0, 'wgrad': 16.0, 'conv_fwd': 35.0, 'conv_wgrad': 16.0}
# Worst ratio |got - ref| / (2^-24 cond) seen on an MI355X (gfx950), by output (test_gemm_f32_fp64_gpu.py::test_worst_ratios prints
# a run's).  A record, not a bound: no K above is derived from it.
GPU_SEEN = {'fwd': 3.68, 'dgrad': 4.90, 'wgrad': 4.90, 'conv_fwd': 4.31, 'conv_wgrad': 3.29}

# route ids (include/tvae_hip.h: tvae_conv1_f32_route, tvae_linear_f32_route)
FWD_GENERIC, FWD_IMG, FWD_IMG_VEC, FWD_IMG_VEC2 = 0, 1, 2, 3
WG_GENERIC, WG_K16, WG_K32, WG_K32_N2 = 0, 1, 2, 3
LIN_GENERIC, LIN_GLDS, LIN_GLDS2, LIN_V4, LIN_NONE = 0, 1, 2, 3, 4
EP_SCALAR, EP_VEC = 0, 1
OP_FWD, OP_DGRAD, OP_WGRAD = 0, 1, 2
# pointer arguments of the dense entry points in header order (the bits of align_mask)
POINTERS = {OP_FWD: ('W', 'X', 'bias', 'gbias', 'res', 'Y'), OP_DGRAD: ('W', 'dpre', 'add', 'aux', 'dX'),
            OP_WGRAD: ('dpre', 'X', 'dW', 'ws')}
F_GBIAS, F_RES, F_MASK, F_ACC = 1, 2, 4, 8


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _v(t, dt, cond):
    return t.double().abs() if cond else t.to(dt)


def ratio(got, ref, cond, k=1.0):
    """Worst (|got - ref| - TINY) / (k 2^-24 cond) over ALL elements.  Where cond is zero the result has to be exact; a non-finite
    result gives inf."""
    got = torch.as_tensor(got).detach().to(ref.device).double().reshape(ref.shape)
    raw = (got - ref).abs()
    err = (raw - TINY).clamp_min(0.0)
    inf = torch.full_like(raw, math.inf)
    r = torch.where(cond > 0, err / (k * UNIT * cond.clamp_min(1e-300)), torch.where(raw > 0, inf, torch.zeros_like(raw)))
    return float(torch.where(torch.isfinite(got), r, inf).max())


def both(fn, *args, **kw):
    return fn(*args, dt=F64, cond=False, **kw), fn(*args, dt=F64, cond=True, **kw)


# ---- the operations -----------------------------------------------------------------------------------------------------
def act_apply(x, act):
    return x if act == 0 else (F.leaky_relu(x, SLOPE) if act == 1 else torch.tanh(x))


def dact(aux, mask, dt=F64, cond=False):
    """act'(aux): mask 1 (lrelu) aux > 0 ? 1 : slope -- +0.0 and -0.0 count as not positive; mask 2 (tanh) 1 - aux aux"""
    a = aux.to(F64 if cond else dt)
    if mask == 1:
        return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))
    return 1 + a * a if cond else 1 - a * a


def fwd(W, X, b, gb, group, res, act, dt=F64, cond=False):
    """W [M][K], X [K][N], b [M] | None, gb [ceil(N / group)][M] | None, res [M][N] | None -> Y [M][N]"""
    pre = _v(W, dt, cond) @ _v(X, dt, cond)
    if b is not None:
        pre = pre + _v(b, dt, cond)[:, None]
    if gb is not None:
        pre = pre + _v(gb, dt, cond)[torch.arange(X.shape[1], device=X.device) // group].t()
    if res is not None:
        pre = pre + _v(res, dt, cond)
    return pre if cond else act_apply(pre, act)


def dgrad(W, d, add, aux, mask, dt=F64, cond=False):
    """W [M][K], d [M][N], add [K][N] | None, aux [K][N] | None (then no mask) -> dX [K][N]"""
    g = _v(W, dt, cond).t() @ _v(d, dt, cond)
    if add is not None:
        g = g + _v(add, dt, cond)
    if aux is not None and mask != 0:
        g = dact(aux, mask, dt, cond) * g
    return g


def wgrad(d, X, init, dt=F64, cond=False):
    """d [M][N], X [K][N], init [M][K] | None -> dW [M][K]"""
    g = _v(d, dt, cond) @ _v(X, dt, cond).t()
    return g if init is None else g + _v(init, dt, cond)


def geom_of(B, Cin, n, k, pad, C, R):
    Ho = n + 2 * pad - k + 1
    return dict(B=B, Cin=Cin, n=n, k=k, pad=pad, C=C, R=R, Ho=Ho, P=Ho * Ho, M=C * R, K=Cin * k * k)


def patches(y, k, pad, dt=F64, cond=False):
    """y [B][Cin][n][n] -> [B][Cin k k][Ho Ho]: the unfold of the zero-padded image, k index (ci, u, v), p index (h, w)"""
    yp = F.pad(_v(y, dt, cond), (pad, pad, pad, pad))
    u = yp.unfold(2, k, 1).unfold(3, k, 1)                         # [B][Cin][Ho][Ho][k][k]
    B, Cin, Ho = u.shape[0], u.shape[1], u.shape[2]
    return u.permute(0, 1, 4, 5, 2, 3).reshape(B, Cin * k * k, Ho * Ho)


def conv_fwd(y, bank, bias, R, k, pad, act, dt=F64, cond=False):
    """y [B][Cin][n][n], bank [C R][Cin k k], bias [C] | None -> out [C][B R Ho Ho] (the layout the kernels write)"""
    cols = patches(y, k, pad, dt, cond)
    B, P, M = cols.shape[0], cols.shape[2], bank.shape[0]
    pre = torch.einsum('mk,bkp->mbp', _v(bank, dt, cond), cols).reshape(M // R, R, B, P).permute(0, 2, 1, 3)
    if bias is not None:
        pre = pre + _v(bias, dt, cond)[:, None, None, None]
    pre = pre.reshape(M // R, B * R * P)
    return pre if cond else act_apply(pre, act)


def conv_wgrad(y, dpre, R, k, pad, dt=F64, cond=False):
    """y [B][Cin][n][n], dpre [C][B R Ho Ho] -> dbank [C R][Cin k k]"""
    cols = patches(y, k, pad, dt, cond)
    B, P, C = cols.shape[0], cols.shape[2], dpre.shape[0]
    dy = _v(dpre, dt, cond).reshape(C, B, R, P).permute(0, 2, 1, 3).reshape(C * R, B, P)
    return torch.einsum('mbp,bkp->mk', dy, cols)


# ---- planted values -----------------------------------------------------------------------------------------------------
def single_positions(Kr):
    """reduction indices of the three one-entry rows: first, last, last before a 16-step boundary"""
    edge = (Kr - 1) // BK * BK - 1 if Kr > BK else Kr // 2
    return [0, Kr - 1, edge]


def plant_rows(A):
    """A [rows][Kr] (a view is fine), in place: rows 0 .. 2 keep ONE entry, row 3 is scaled by 2^-20"""
    rows, Kr = A.shape
    for r, kk in enumerate(single_positions(Kr)):
        if r < rows:
            A[r] = 0.0
            A[r, kk] = (r + 1) / 3.0                               # full-mantissa values
    if rows > 3:
        A[3] *= 2.0 ** -20
    return A


AUX_PLANTS = (0.0, -0.0, 1e-30, -1e-30)


def plant_aux(aux):
    """+0.0, -0.0, 1e-30, -1e-30 in turn at rows 0, 63, 64, 127 x columns 0, 31, 32, 127 (those inside the tensor)"""
    i = 0
    for r in (0, 63, 64, 127):
        for c in (0, 31, 32, 127):
            if r < aux.shape[0] and c < aux.shape[1]:
                aux[r, c] = AUX_PLANTS[i % 4]
                i += 1
    return aux


def strided(t, ld, fill=PAD_IN):
    """[rows][N] -> a contiguous [rows][ld] tensor holding t in its first N columns and `fill` in the pad columns"""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def blank(rows, N, ld, device=None):
    """an output: NaN where the kernel has to write, SENTINEL in the pad columns"""
    out = torch.full((rows, ld), SENTINEL, device=device)
    out[:, :N] = math.nan
    return out


# ---- dense cases --------------------------------------------------------------------------------------------------------
def _dc(name, M, N, K, main, ep, pa=0, pb=0, act=0, group=0, res=False, mis=None, aux=True):
    """pa / pb: pad columns of ld_a / ld_b (fwd: ldx, ldy; dgrad: ldd, ldx); act: activation (fwd) or mask (dgrad); res: res / add
    given; mis: the pointer offset by one float; aux=False: dgrad called with aux = NULL (its mask is then ignored)"""
    return dict(name=name, M=M, N=N, K=K, main=main, ep=ep, pa=pa, pb=pb, act=act, group=group, res=res, mis=mis, aux=aux)


FWD_CASES = [
    _dc('generic_129_127_17', 129, 127, 17, LIN_GENERIC, EP_SCALAR, 1, 1, act=1, group=100, res=True),
    _dc('generic_127_129_15', 127, 129, 15, LIN_GENERIC, EP_SCALAR, act=2),
    _dc('generic_ldx_odd', 128, 128, 16, LIN_GENERIC, EP_SCALAR, 1, 0, act=1),
    _dc('generic_nine_tiles', 128, 1152, 17, LIN_GENERIC, EP_SCALAR, 0, 4, act=1, res=True),
    _dc('generic_gbias128_res', 129, 256, 17, LIN_GENERIC, EP_SCALAR, 4, 0, act=2, group=128, res=True),
    _dc('glds_vec_nine_tiles', 128, 1152, 16, LIN_GLDS, EP_VEC, act=1),
    _dc('glds_vec_pad4_res', 128, 128, 16, LIN_GLDS, EP_VEC, 4, 4, act=2, res=True),
    _dc('glds_vec_pad64', 256, 128, 32, LIN_GLDS, EP_VEC, 64, 64, act=0),
    _dc('glds_scalar_gbias128', 256, 256, 16, LIN_GLDS, EP_SCALAR, act=1, group=128),
    _dc('glds_scalar_gbias100_res', 128, 256, 16, LIN_GLDS, EP_SCALAR, 4, 64, act=2, group=100, res=True),
    _dc('glds_scalar_ldy_odd', 128, 128, 16, LIN_GLDS, EP_SCALAR, 0, 1, act=0, res=True),
    _dc('glds_scalar_nine_tiles', 128, 1152, 16, LIN_GLDS, EP_SCALAR, 0, 1, act=1),
    _dc('mis_W', 128, 128, 16, LIN_GENERIC, EP_SCALAR, act=1, res=True, mis='W'),
    _dc('mis_X', 128, 128, 16, LIN_GENERIC, EP_SCALAR, act=1, res=True, mis='X'),
    _dc('mis_bias', 128, 128, 16, LIN_GLDS, EP_VEC, act=1, res=True, mis='bias'),
    _dc('mis_gbias', 128, 128, 16, LIN_GLDS, EP_SCALAR, act=1, group=100, mis='gbias'),
    _dc('mis_res', 128, 128, 16, LIN_GLDS, EP_SCALAR, act=1, res=True, mis='res'),
    _dc('mis_Y', 128, 128, 16, LIN_GLDS, EP_SCALAR, act=1, res=True, mis='Y'),
]

DGRAD_CASES = [      # M = the reduction, K = the output rows
    _dc('generic_17_127_129', 17, 127, 129, LIN_GENERIC, EP_SCALAR, 1, 1, act=1, res=True),
    _dc('generic_15_129_127', 15, 129, 127, LIN_GENERIC, EP_SCALAR, act=2),
    _dc('generic_ldd_odd', 16, 128, 128, LIN_GENERIC, EP_SCALAR, 1, 0, act=1),
    _dc('generic_nine_tiles', 17, 1152, 128, LIN_GENERIC, EP_SCALAR, 0, 4, act=1, res=True),
    _dc('glds2_vec_nine_tiles', 16, 1152, 128, LIN_GLDS2, EP_VEC, act=1, res=True),
    _dc('glds2_vec_pad4_tanh', 16, 128, 128, LIN_GLDS2, EP_VEC, 4, 4, act=2),
    _dc('glds2_vec_pad64_nomask_add', 32, 128, 256, LIN_GLDS2, EP_VEC, 64, 64, act=0, res=True),
    _dc('glds2_vec_nomask', 16, 128, 128, LIN_GLDS2, EP_VEC, act=0),
    _dc('glds2_vec_aux_null', 16, 128, 128, LIN_GLDS2, EP_VEC, act=1, res=True, aux=False),
    _dc('glds2_scalar_ldx_odd', 16, 128, 128, LIN_GLDS2, EP_SCALAR, 0, 1, act=1, res=True),
    _dc('glds2_scalar_tanh_add', 16, 256, 128, LIN_GLDS2, EP_SCALAR, 4, 1, act=2, res=True),
    _dc('glds2_scalar_nine_tiles', 16, 1152, 128, LIN_GLDS2, EP_SCALAR, 0, 1, act=1),
    _dc('mis_W', 16, 128, 128, LIN_GENERIC, EP_SCALAR, act=1, res=True, mis='W'),
    _dc('mis_dpre', 16, 128, 128, LIN_GENERIC, EP_SCALAR, act=1, res=True, mis='dpre'),
    _dc('mis_add', 16, 128, 128, LIN_GLDS2, EP_SCALAR, act=1, res=True, mis='add'),
    _dc('mis_aux', 16, 128, 128, LIN_GLDS2, EP_SCALAR, act=1, res=True, mis='aux'),
    _dc('mis_dX', 16, 128, 128, LIN_GLDS2, EP_SCALAR, act=1, res=True, mis='dX'),
]

# weight gradient: (name, M, N, K, pad of ldd, pad of ldx, main, slices with a large workspace)
WGRAD_CASES = [
    dict(name='v4_17_slices', M=128, N=1088, K=128, pa=4, pb=64, main=LIN_V4, slices=17),
    dict(name='generic_13_slices_ragged', M=128, N=1000, K=128, pa=1, pb=4, main=LIN_GENERIC, slices=13),
    dict(name='generic_130_777_70', M=130, N=777, K=70, pa=0, pb=3, main=LIN_GENERIC, slices=10),
    dict(name='mis_dpre', M=128, N=1088, K=128, pa=0, pb=0, main=LIN_GENERIC, slices=17, mis='dpre'),
    dict(name='mis_X', M=128, N=1088, K=128, pa=0, pb=0, main=LIN_GENERIC, slices=17, mis='X'),
]
WS_KINDS = ('large', 'two', 'one', 'none')       # workspace: plenty, exactly two slabs, one slab (no split), NULL


def ws_floats(kind, per):
    return {'large': 64 * per, 'two': 2 * per, 'one': per, 'none': 0}[kind]


def dense_flags(op, c, acc=0):
    if op == OP_FWD:
        return (F_GBIAS if c['group'] else 0) | (F_RES if c['res'] else 0)
    if op == OP_DGRAD:
        return (F_RES if c['res'] else 0) | (F_MASK if c['act'] and c['aux'] else 0)
    return F_ACC if acc else 0


def dense_align(op, c):
    """align_mask of a case: every pointer 16-byte aligned except the one the case offsets by a float"""
    names = POINTERS[op]
    return sum(1 << i for i, nm in enumerate(names) if nm != c.get('mis'))


def dense_route_args(op, c, ws=0, acc=0):
    """arguments of tvae_linear_f32_route up to `which`"""
    if op == OP_WGRAD:
        return (op, c['M'], c['N'], c['K'], c['N'] + c['pa'], c['N'] + c['pb'], dense_align(op, c), dense_flags(op, c, acc), ws)
    return (op, c['M'], c['N'], c['K'], c['N'] + c['pa'], c['N'] + c['pb'], dense_align(op, c), dense_flags(op, c), 0)


def fwd_tensors(c, seed=100):
    M, N, K_ = c['M'], c['N'], c['K']
    W = plant_rows(rnd(M, K_, seed=seed + 1, scale=K_ ** -0.5))
    X, b = rnd(K_, N, seed=seed + 2), rnd(M, seed=seed + 3)
    gb = rnd((N + c['group'] - 1) // c['group'], M, seed=seed + 4) if c['group'] else None
    res = rnd(M, N, seed=seed + 5) if c['res'] else None
    if res is not None:                  # the last row's pre-activations: within rounding of 0
        res[M - 1] = -fwd(W, X, b, gb, c['group'], None, 0, dt=F32)[M - 1]
    return dict(W=W, X=X, bias=b, gbias=gb, res=res)


def fwd_ref(c, t, **kw):
    return fwd(t['W'], t['X'], t['bias'], t['gbias'], c['group'], t['res'], c['act'], **kw)


def dgrad_tensors(c, seed=200):
    M, N, K_ = c['M'], c['N'], c['K']
    W = rnd(M, K_, seed=seed + 1, scale=M ** -0.5)
    plant_rows(W.t())                    # the A operand of the data gradient is W^T: its rows are W's columns
    d = rnd(M, N, seed=seed + 2)
    add = rnd(K_, N, seed=seed + 4) if c['res'] else None
    aux = plant_aux(rnd(K_, N, seed=seed + 3).clamp(-0.9, 0.9)) if c['aux'] else None
    return dict(W=W, dpre=d, add=add, aux=aux)


def dgrad_ref(c, t, **kw):
    return dgrad(t['W'], t['dpre'], t['add'], t['aux'], c['act'], **kw)


def wgrad_tensors(c, seed=300):
    M, N, K_ = c['M'], c['N'], c['K']
    d = plant_rows(rnd(M, N, seed=seed + 1))
    X = rnd(K_, N, seed=seed + 2)
    X[K_ // 2] *= 2.0 ** -20
    return dict(dpre=d, X=X, init=rnd(M, K_, seed=seed + 3))


def wgrad_ref(c, t, acc, **kw):
    return wgrad(t['dpre'], t['X'], t['init'] if acc else None, **kw)


# ---- convolution cases ----------------------------------------------------------------------------------------------------
# forward: (name, (B, Cin, n, k, pad, C, R), act, route)
CONV_FWD_CASES = [
    ('img_ragged_tile', (2, 1, 12, 5, 2, 3, 4), 1, FWD_IMG),                    # P = 144: a ragged second tile
    ('img_vec', (2, 1, 12, 4, 1, 8, 16), 2, FWD_IMG_VEC),
    ('img_vec_cin3', (2, 3, 12, 4, 1, 8, 16), 0, FWD_IMG_VEC),
    ('img_vec2', (2, 1, 12, 4, 1, 16, 16), 1, FWD_IMG_VEC2),
    ('img_vec_three_row_tiles', (2, 1, 12, 4, 1, 24, 16), 0, FWD_IMG_VEC),      # M = 384
    ('generic_cin3', (2, 3, 108, 100, 0, 2, 4), 1, FWD_GENERIC),                # K = 30 000
    ('generic_cin3_ragged_k', (2, 3, 108, 99, 0, 2, 4), 2, FWD_GENERIC),        # K = 29 403 = 11 (mod 16)
    ('generic_cin1', (2, 1, 160, 180, 16, 2, 4), 2, FWD_GENERIC),               # K = 32 400
    ('generic_cin1_ragged_k', (2, 1, 160, 179, 16, 2, 4), 1, FWD_GENERIC),      # K = 32 041 = 9 (mod 16)
    ('generic_m256', (2, 3, 108, 100, 0, 16, 16), 0, FWD_GENERIC),
    ('pad_only_tiles_k1', (2, 1, 8, 1, 12, 2, 4), 0, FWD_IMG),                  # tiles that meet only padding: act(bias) exactly
    ('nk0_tiles', (2, 1, 8, 4, 12, 2, 4), 1, FWD_IMG),                          # ... and tiles whose k range is EMPTY (nk == 0)
    ('r1', (2, 1, 12, 5, 2, 5, 1), 2, FWD_IMG),
    ('two_exact_tiles', (2, 1, 20, 7, 1, 2, 4), 0, FWD_IMG),                    # Ho = 16, P = 256
    ('zero_skip_both_ends', (2, 1, 20, 16, 8, 2, 4), 1, FWD_IMG),               # kbeg > 0 and kstop < K in one launch
]

# weight gradient: (name, (B, Cin, n, k, pad, C, R), route, {workspace kind: (slices, images per slice)})
CONV_WGRAD_CASES = [
    ('k32_n2_xcd_map', (8, 1, 20, 16, 3, 2, 4), WG_K32_N2, {'large': (8, 1), 'two': (2, 4), 'none': (1, 8)}),
    ('k32_n2_uneven_slices', (5, 1, 20, 16, 3, 2, 4), WG_K32_N2, {'large': (5, 1), 'two': (2, 3), 'none': (1, 5)}),
    ('k32_m12', (8, 1, 12, 5, 2, 3, 4), WG_K32, {'large': (8, 1), 'two': (2, 4), 'none': (1, 8)}),
    ('k32_m256', (8, 1, 12, 5, 2, 64, 4), WG_K32, {'large': (8, 1), 'two': (2, 4), 'none': (1, 8)}),
    ('k32_partial_image', (8, 1, 20, 13, 2, 2, 4), WG_K32, {'large': (8, 1), 'two': (2, 4), 'none': (1, 8)}),   # n0 > 0: ulo = 9
    ('k16_cin3', (3, 3, 40, 9, 4, 2, 4), WG_K16, {'large': (3, 1), 'two': (2, 2), 'none': (1, 3)}),
    ('k16_cin1', (3, 1, 64, 9, 4, 2, 4), WG_K16, {'large': (3, 1), 'two': (2, 2), 'none': (1, 3)}),
    ('generic_338_slices', (2, 3, 100, 5, 4, 2, 4), WG_GENERIC, {'large': (338, 0), 'two': (2, 0), 'none': (1, 0)}),
    ('generic_cin1', (2, 1, 180, 5, 4, 2, 4), WG_GENERIC, {'large': (847, 0), 'two': (2, 0), 'none': (1, 0)}),
    ('r1', (5, 1, 12, 5, 2, 5, 1), WG_K32, {'large': (5, 1), 'two': (2, 3), 'none': (1, 5)}),
    ('one_tap', (2, 1, 8, 1, 12, 2, 4), WG_K32, {'large': (2, 1), 'two': (2, 1), 'none': (1, 2)}),             # N = 1
]
CONV_WS_KINDS = ('large', 'two', 'none')


def conv_ws_floats(kind, per):
    return {'large': 1100 * per, 'two': 2 * per, 'none': 0}[kind]


def conv_fwd_tensors(geom, seed=400):
    g = geom_of(*geom)
    y = torch.rand(g['B'], g['Cin'], g['n'], g['n'], generator=torch.Generator().manual_seed(seed + 1))
    bank = plant_rows(rnd(g['M'], g['K'], seed=seed + 2, scale=g['K'] ** -0.5))
    return dict(y=y, bank=bank, bias=rnd(g['C'], seed=seed + 3, scale=0.1))


def conv_fwd_ref(geom, act, t, **kw):
    g = geom_of(*geom)
    return conv_fwd(t['y'], t['bank'], t['bias'], g['R'], g['k'], g['pad'], act, **kw)


def conv_wgrad_tensors(geom, seed=500):
    g = geom_of(*geom)
    y = torch.rand(g['B'], g['Cin'], g['n'], g['n'], generator=torch.Generator().manual_seed(seed + 1))
    dy = plant_rows(rnd(g['M'], g['B'] * g['P'], seed=seed + 2))          # [c R + r][(img, p)]: the A operand, reduction order
    dpre = dy.view(g['C'], g['R'], g['B'], g['P']).permute(0, 2, 1, 3).reshape(g['C'], -1).contiguous()
    return dict(y=y, dpre=dpre)


def conv_wgrad_ref(geom, t, **kw):
    g = geom_of(*geom)
    return conv_wgrad(t['y'], t['dpre'], g['R'], g['k'], g['pad'], **kw)


def conv_fwd_tile_ranges(geom):
    """(kbeg, kstop, nk) of every position tile of one image in conv1_fwd_img_kernel, from the formula its header documents: tap
    row u only meets image rows h + u - pad in [0, n) for the tile's output rows [hmin, hmax]; the kept taps are rounded outwards
    to the 16-step.  Cin > 1: no skipping."""
    g = geom_of(*geom)
    out = []
    for p0 in range(0, g['P'], BN):
        kbeg, kstop = 0, g['K']
        if g['Cin'] == 1:
            hmin, hmax = p0 // g['Ho'], min(g['P'] - 1, p0 + BN - 1) // g['Ho']
            ulo, uhi = max(0, g['pad'] - hmax), min(g['k'] - 1, g['pad'] + g['n'] - 1 - hmin)
            kbeg = ulo * g['k'] // BK * BK
            kstop = max(kbeg, min(g['K'], ((uhi + 1) * g['k'] + BK - 1) // BK * BK))
        out.append((kbeg, kstop, (kstop - kbeg + BK - 1) // BK))
    return out
