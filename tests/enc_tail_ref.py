"""float64 restatements of the encoder tail (conv2 1x1x1 + the stacked head projection: csrc/enc_tail_x6_kernels.hpp,
enc_tail_wide_kernels.hpp, enc_tail_wgrad_kernels.hpp behind abi_enc_tail_x6.hip / abi_enc_tail_wide.hip) --
tvae_enc_tail_fwd_x6 / _dgrad_x6 / _wgrad_x6, tvae_enc_tail_fwd_wide / _dgrad_wide / _wgrad_wide and the slab total behind both
weight gradients -- with the condition quantities and floors of their error bounds and the cases both
test_enc_tail_ref_cpu.py (which measures K on CPU arithmetic) and test_enc_tail_fp64_gpu.py run.  A plain helper module; it
works on whatever device its arguments live on (the GPU file forms the two large references in float64 torch on the device).

Every operation is ONE expression in the dtype `dt`: float64 is the reference, cond=True evaluates the same expression on the
absolute values of its operands -- the per-element CONDITION QUANTITY, the sum of the absolute values of the terms added.

    forward          H = act(W2 A1 + b2)            cond_H     = |W2| |A1| + |b2|
                     heads = Wh H + bh              cond_heads = |Wh| cond_H + |bh|   (the kernels project their OWN rounded H)
    data gradient    dH  = mH . (Wh^T dheads)       cond_dH    = mH . (|Wh^T| |dheads|)
    (GIVEN words)    dA1 = mA . (W2^T dH)           cond_dA1   = mA . (|W2^T| cond_dH)          m = bit ? 1 : fp32(0.01)
    weight gradient  dW2 = dH A1^T, dW = D A^T      cond       = sum_n |.| |.|   (dH from the words; cond_dH in its place)

The activations are 1-Lipschitz, so the error of the pre-activation carries over at most 1 : 1 and cond_H is the pre-activation's;
tanhf's own error (a few ulp of |H| <= |pre| <= cond_H) lies inside K >= 16, as in mlp_ends_ref's first decoder layer.

A kernel result `got` has to satisfy, in EVERY element,

    |got - ref| <= K[name] * UNIT[parts] * cond + floor,         exactly where cond == 0 (floor or not).

UNIT, from the mantissa bits the split code keeps (csrc/conv_x6_device.hpp, dense_x6_kernels.hpp):
  parts = 3  split3x8: three bf16 parts hold all 24 bits, six products in fp32 accumulators: fp32 arithmetic, UNIT = 2^-24.
  parts = 2  split2hx8 on the scaled value y: h = fp16(y) keeps 11 bits, |y - h| <= 2^-11 |y|; y - h is exact in fp32 with at most
             13 bits, of which l = fp16(y - h) keeps 11: |y - h - l| <= 2^-11 |y - h| <= 2^-22 |y|.  mfma3h issues h h', h l', l h'
             (each exact in the fp32 accumulator) and leaves out l l' <= 2^-22 |y y'|.  Per product
             2^-22 (y) + 2^-22 (y') + 2^-22 (l l') = 3 * 2^-22 = UNIT[2]; the fp32 accumulation adds 2^-24 per term as ever.
  parts = 1  bf16_pair: one bf16 number of 8 bits per operand, 2^-9 each; per product 2^-9 + 2^-9 + 2^-18 = UNIT[1].

FLOOR (parts = 2 only; besides it TINY = 2^-119 everywhere: 128 products that underflow fp32's normal range).  An operand is
multiplied by the power of two s = h3_scale(amax) of its scale group, 2^14 <= s amax < 2^15 (restated below bit for bit), and
fp16's subnormal spacing is 2^-24.  Where |y - h| < 2^-14 -- elements 2^-17 and more below their group's maximum -- l is
rounded to a multiple of 2^-24 instead of to 11 bits: |y - h - l| <= 2^-25 of the SCALED value.  Where |y| < 2^-14 as well, h
is such a multiple itself, |y - h| <= 2^-25, and l = fp16(y - h) is 0 or cancels it: again at most 2^-25 is lost.  So an
element of a group with scale s is represented to delta(s) = 2^-25 / s absolutely, besides UNIT relatively (with the maximum
of the group at least 2^14 / s that is 2^-39 of it, the figure of csrc/conv_x6_device.hpp), and a product sum_k w_k x_k gains

    floor = delta_w sum_k |x_k| + delta_x sum_k |w_k|                                   (mm_floor)

with the scale groups of the kernels: rows of every weight from their own maximum (tvae_dense_split2h's trailer); A1 of the
forwards under ONE scale from the largest of the amax_a1 words; dheads of the wide data gradient under the amax_dheads word;
the operand of every SECOND GEMM (H, G, dH in registers) under the exact scale of its 128 x 32 chunk -- taken here from the
reference's chunk maximum, DOUBLED because the kernel's own maximum may lie just across a power of two; the weight
gradients: A per channel from amax_a1 / amax_a, dH of wgrad_x6 per row from fp32(max |dheads| * sum_h |Wh[h][row]|), D of
wgrad_wide from amax_d.  Floors carry through the chain like errors: |Wh| floor_H into the heads, mA |W2^T| floor_dH into dA1.

K: never from the kernels.  CPU arithmetic against this file on every case below (test_enc_tail_ref_cpu.py::
test_budget_constants measures and prints them): parts = 3 fp32 torch; parts = 2 / 1 a torch emulation of the operand rounding
(fp16 / bf16 casts under the same scales, fp32 products and sums: emu_mm).  K = max(16, 8 x worst ratio) per output, the ratio
in units of UNIT[parts] (floor taken off first), worst over the parts:

    output       ratio   8 x     K      by parts (3 | 2 | 1)        output       ratio   8 x     K      by parts (2 | 1)
    x6_H         6.933  55.46   56      6.933 | 0.616 | 1.093       wide_H       1.093   8.74   16      0.616 | 1.093
    x6_heads     1.206   9.65   16      1.206 | 0.218 | 0.055       wide_heads   0.211   1.69   16      0.129 | 0.211
    x6_dA1      12.061  96.49   97     12.061 | 1.375 | 1.651       wide_dH      1.416  11.33   16      0.372 | 1.416
    x6_dW2       9.124  72.99   73      9.124 | 1.051 | 1.394       wide_dA1     1.180   9.44   16      0.575 | 1.180
                                                                    wide_dW      0.463   3.70   16      0.463

(The fp32 figures of the x6 family are worst cases over the 17 M elements of the two large cases and of chains of two sums.)

Planted values (what a wrong kernel cannot hide behind a 128-term condition quantity): W2 has a row and a column with ONE
entry, so H[9] = act(w A1[77]) and dA1[40] = mA w dH[21] are single products; A1[77], dheads[0] and one column of the weight
gradient's A hold FULL-mantissa values whose third bf16 part is as large as it gets (dropped: 2^-17 = 128 UNIT[3]); A1 carries
+-0, +-1e-30, +-1e-40 at the edges of chunks, words and of et_row's map, and an all-zero column that meets b2 = 0.
"""
import functools
import math

import torch

F64, F32 = torch.float64, torch.float32
C = 128
SLOPE = float(torch.tensor(0.01, dtype=F32))                  # what the kernels get: fp32(0.01)
UNIT = {3: 2.0 ** -24, 2: 3 * 2.0 ** -22, 1: 2.0 ** -8 + 2.0 ** -18}
TINY = 2.0 ** -119
SENTINEL = -7777.0            # prefill of strided outputs: pad columns must come back holding it
PAD_IN = 1e30                 # pad columns of strided inputs: a read of one shows in the result
BITS_PREFILL = 0xA5A5A5A5 - (1 << 32)                        # prefill of sign-word outputs, as int32
PADS = (1, 4, 7, 64)          # lda / ldh / ldo / ldd beyond N in the forward and data-gradient cases

K = {'x6_H': 56.0, 'x6_heads': 16.0, 'x6_dA1': 97.0, 'x6_dW2': 73.0, 'wide_H': 16.0, 'wide_heads': 16.0, 'wide_dH': 16.0,
     'wide_dA1': 16.0, 'wide_dW': 16.0}
# Worst ratio (error - floor) / (UNIT[parts] cond) seen on an MI355X (gfx950), by output
# (test_enc_tail_fp64_gpu.py::test_worst_ratios prints a run's).  A record, not a bound: no K above is derived from it.
GPU_SEEN = {'x6_H': 6.35, 'x6_heads': 0.769, 'x6_dA1': 8.70, 'x6_dW2': 5.12, 'wide_H': 1.09, 'wide_heads': 0.211, 'wide_dH': 1.42,
            'wide_dA1': 1.18, 'wide_dW': 0.271}
# ... by parts (3 | 2 | 1): x6_H 6.35 | 0.372 | 1.09, x6_heads 0.769 | 0.127 | 0.055, x6_dA1 8.70 | 0.684 | 1.65, x6_dW2 5.12 | 0.616 |
# 1.39; (2 | 1): wide_H 0.372 | 1.09, wide_heads 0.092 | 0.211, wide_dH 0.393 | 1.42, wide_dA1 0.423 | 1.18, wide_dW 0.271


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _v(t, dt, cond):
    return t.double().abs() if cond else t.to(dt)


def ratio(got, ref, cond, unit, floor=None):
    """Worst (|got - ref| - floor - TINY) / (unit cond) over ALL elements.  Where cond is zero the result has to be exact,
    whatever the floor; a non-finite result gives inf."""
    got = torch.as_tensor(got).detach().to(ref.device).double().reshape(ref.shape)
    raw = (got - ref).abs()
    err = (raw - TINY - (0.0 if floor is None else floor)).clamp_min(0.0)
    inf = torch.full_like(raw, math.inf)
    r = torch.where(cond > 0, err / (unit * cond.clamp_min(1e-300)), torch.where(raw > 0, inf, torch.zeros_like(raw)))
    return float(torch.where(torch.isfinite(got), r, inf).max())


# ---- sign words (include/tvae_hip.h: [N][4] uint32, bit (r & 31) of word r >> 5 of column n is row r) ---------------------------
def pack(bits):
    """bool [128][N] -> int32 [N][4]"""
    b = bits.t().reshape(-1, 4, 32).to(torch.int64)
    w = (b << torch.arange(32, device=bits.device)).sum(2)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack(words):
    """int32 [N][4] -> bool [128][N]"""
    w = words.to(torch.int64)[:, :, None]
    return ((w >> torch.arange(32, device=words.device)) & 1).bool().reshape(-1, 128).t().contiguous()


BIT_PATTERNS = ['random', 'zeros', 'ones', 'walk', 'cowalk']


def bit_pattern(kind, N, seed):
    """bool [128][N]: random words (drawn as dense_bits_ref.random_bits draws them), all zero, all one, a walking one (column n
    has only bit n % 128), its complement."""
    if kind == 'random':
        g = torch.Generator().manual_seed(seed)
        return unpack(torch.randint(-2 ** 31, 2 ** 31, (N, 4), generator=g, dtype=torch.int64).to(torch.int32))
    if kind in ('zeros', 'ones'):
        return torch.full((C, N), kind == 'ones')
    walk = torch.arange(C)[:, None] == (torch.arange(N) % C)[None, :]
    return walk if kind == 'walk' else ~walk


def perm():
    """k-column order of the second GEMM's weight (include/tvae_hip.h): slot 16 u + 8 h + j <- row 16 u + 8 (j >> 2) + 4 h + (j & 3)"""
    return torch.tensor([16 * u + 8 * (j >> 2) + 4 * h + (j & 3) for u in range(8) for h in range(2) for j in range(8)])


# ---- the operations ---------------------------------------------------------------------------------------------------------
def act_apply(x, act):
    return x if act == 0 else (torch.nn.functional.leaky_relu(x, SLOPE) if act == 1 else torch.tanh(x))


def mask(bits, dt=F64):
    return torch.where(bits, torch.ones((), dtype=dt, device=bits.device), torch.full((), SLOPE, dtype=dt, device=bits.device))


def fwd(W2, A1, b2, Wh, bh, act, dt=F64, cond=False):
    """W2 [128][128], A1 [128][N], b2 [128] or None, Wh [nh][128], bh [nh] -> {H [128][N], heads [nh][N]}"""
    pre = _v(W2, dt, cond) @ _v(A1, dt, cond)
    if b2 is not None:
        pre = pre + _v(b2, dt, cond)[:, None]
    H = pre if cond else act_apply(pre, act)
    return {'H': H, 'heads': _v(Wh, dt, cond) @ H + _v(bh, dt, cond)[:, None]}


def heads_of(Wh, H, bh, dt=F64, cond=False):
    """The head rows from a GIVEN (stored) H."""
    return _v(Wh, dt, cond) @ _v(H, dt, cond) + _v(bh, dt, cond)[:, None]


def dgrad(W2, Wh, dheads, bits_h, bits_a, dt=F64, cond=False):
    """dheads [nh][N], bits_* bool [128][N] -> {dH, dA1} [128][N]"""
    dH = mask(bits_h, F64 if cond else dt) * (_v(Wh, dt, cond).t() @ _v(dheads, dt, cond))
    return {'dH': dH, 'dA1': mask(bits_a, F64 if cond else dt) * (_v(W2, dt, cond).t() @ dH)}


def wgrad(D, A, dt=F64, cond=False):
    """D [rows][N], A [128][N] -> dW [rows][128]"""
    return _v(D, dt, cond) @ _v(A, dt, cond).t()


def both(fn, *args):
    return fn(*args, dt=F64, cond=False), fn(*args, dt=F64, cond=True)


# ---- h3 scales and floors ---------------------------------------------------------------------------------------------------
def h3_scale(amax):
    """csrc/conv_x6_device.hpp:h3_scale on the bit pattern of an fp32 tensor: the power of two s with 2^14 <= s amax < 2^15."""
    e = (amax.to(F32).contiguous().view(torch.int32) >> 23) & 0xff
    e = torch.where(e == 0, torch.full_like(e, 127), e)
    return torch.pow(2.0, ((268 - e).clamp(2, 252) - 127).double())


def delta(amax):
    return 2.0 ** -25 / h3_scale(amax)


def chunk_max(T):
    """[rows][N] -> [N]: max |T| over the aligned 32-column chunk (all rows) of every column"""
    N = T.shape[1]
    m = T.abs().amax(0)
    m = torch.cat([m, m.new_zeros(-N % 32)]).view(-1, 32).amax(1)
    return m.repeat_interleave(32)[:N]


def mm_floor(W, X, dw, dx):
    """floor of sum_k W[m][k] X[k][n]: dw [M] (or scalar) per row of W, dx [N] (or scalar) per column of X"""
    W, X = W.double().abs(), X.double().abs()
    dw = torch.as_tensor(dw, dtype=F64, device=W.device).expand(W.shape[0])
    dx = torch.as_tensor(dx, dtype=F64, device=W.device).expand(X.shape[1])
    return dw[:, None] * X.sum(0)[None, :] + W.sum(1)[:, None] * dx[None, :]


def rowmax(W):
    return W.abs().amax(1)


def fwd_floor(wide, W2, A1, Wh, amax_a1, H):
    """parts = 2: floors of {H, heads}; H = the reference H (wide: its chunk maxima scale the second GEMM)"""
    fH = mm_floor(W2, A1, delta(rowmax(W2)), delta(amax_a1.max()))
    fh = Wh.double().abs() @ fH
    if wide:
        fh = fh + mm_floor(Wh, H, delta(rowmax(Wh)), 2 * delta(chunk_max(H)))
    return {'H': fH, 'heads': fh}


def dgrad_floor(wide, W2, Wh, dheads, bits_h, bits_a, amax_d, ref):
    """parts = 2: floors of {dH, dA1}; ref = dgrad(...) in float64"""
    mH, mA = mask(bits_h), mask(bits_a)
    G = Wh.double().t() @ dheads.double()
    if wide:
        fdH = mH * mm_floor(Wh.t(), dheads, delta(rowmax(Wh.t())), delta(amax_d))
        second = chunk_max(ref['dH'])
    else:
        fdH = torch.zeros_like(G)                          # the skinny GEMM of the x6 family stays in the exact split
        second = chunk_max(G)                              # ... and its chunk scale comes from G BEFORE the mask
    f2 = mm_floor(W2.t(), ref['dH'], delta(rowmax(W2.t())), 2 * delta(second))
    return {'dH': fdH, 'dA1': mA * (W2.double().abs().t() @ fdH + f2)}


def wgrad_x6_scale_d(Wh, dheads):
    """fp32(max |dheads| * rs), rs = the fp32 sum of |Wh[h][row]| in h order, as enc_tail_wgrad_x6_kernel forms it"""
    rs = torch.zeros(C)
    for h in range(Wh.shape[0]):
        rs = rs + Wh[h].abs()
    return dheads.abs().max() * rs


def wgrad_floor(D, A, amax_d, amax_a):
    return mm_floor(D, A.t(), delta(amax_d), delta(amax_a))


# ---- CPU emulation of the operand rounding (K of parts = 2 / 1) ---------------------------------------------------------------
def emu_mm(parts, W, X, sw=None, sx=None):
    """W [M][K] @ X [K][N] in fp32 with the operands rounded as `parts` rounds them; sw [M] / sx [N] (or scalars): h3 scales"""
    W, X = W.float(), X.float()
    if parts == 3:
        return W @ X
    if parts == 1:
        return W.bfloat16().float() @ X.bfloat16().float()
    sw = torch.as_tensor(sw, dtype=F32).expand(W.shape[0])[:, None]
    sx = torch.as_tensor(sx, dtype=F32).expand(X.shape[1])[None, :]
    yw, yx = W * sw, X * sx
    hw, hx = yw.half().float(), yx.half().float()
    lw, lx = (yw - hw).half().float(), (yx - hx).half().float()
    return ((hw @ hx + hw @ lx + lw @ hx) / sw) / sx


def emu_fwd(parts, wide, W2, A1, b2, Wh, bh, act, amax_a1):
    s = (lambda a: h3_scale(a).float()) if parts == 2 else (lambda a: None)
    pre = emu_mm(parts, W2, A1, s(rowmax(W2)), s(amax_a1.max()) if parts == 2 else None)
    H = act_apply(pre if b2 is None else pre + b2[:, None], act)
    if wide:
        heads = emu_mm(parts, Wh, H, s(rowmax(Wh)), s(chunk_max(H))) + bh[:, None]
    else:
        heads = Wh @ H + bh[:, None]
    return {'H': H, 'heads': heads}


def emu_dgrad(parts, wide, W2, Wh, dheads, bits_h, bits_a, amax_d):
    s = (lambda a: h3_scale(a).float()) if parts == 2 else (lambda a: None)
    if wide:
        G = emu_mm(parts, Wh.t(), dheads, s(rowmax(Wh.t())), s(amax_d))
    else:
        G = emu_mm(3 if parts == 2 else parts, Wh.t(), dheads)
    dH = mask(bits_h, F32) * G
    dA1 = mask(bits_a, F32) * emu_mm(parts, W2.t(), dH, s(rowmax(W2.t())), s(chunk_max(dH if wide else G)))
    return {'dH': dH, 'dA1': dA1}


def emu_wgrad(parts, D, A, amax_d, amax_a):
    s = (lambda a: h3_scale(a).float()) if parts == 2 else (lambda a: None)
    return emu_mm(parts, D, A.t(), s(amax_d), s(amax_a))


# ---- grid arithmetic of the kernels, restated (abi_enc_tail_*.hip: et_grid; the kernels' chunk loops) -----------------------------
def et_waves(N, cus):
    """my of every wave of the forward / data-gradient grid: the chunks wave gw runs (0: it returns at once)"""
    nchunks = (N + 31) // 32
    grid = min((nchunks + 7) // 8, cus)
    gstride = 8 * grid
    return [(nchunks - 1 - gw) // gstride + 1 if gw < nchunks else 0 for gw in range(gstride)]


def ew_counts(nchunks, cus):
    """chunks of every workgroup of the weight-gradient grid"""
    grid = min(nchunks, cus)
    per = (nchunks + grid - 1) // grid
    return [max(0, min(per, nchunks - b * per)) for b in range(grid)]


def wide_rems(kx):
    """rem of the eight k-steps of the wide kernel's first GEMM"""
    return [kx - 16 * t for t in range(8)]


def wide_tiles(m2):
    """(halves run, row tiles stored) of the wide kernel's second GEMM"""
    return [64 * hf < m2 for hf in range(2)], [32 * i < m2 for i in range(4)]


# ---- cases ------------------------------------------------------------------------------------------------------------------
NS_SMALL = [1, 31, 32, 33, 255, 256, 257]


def ns_big(cus):
    """a few waves run two chunks (one of them ragged), the rest one | three chunks against two"""
    return [32 * (8 * cus + 3) + 5, 32 * (16 * cus + 8)]


PLANT_ROWS = [0, 3, 4, 7, 8, 31, 32, 127]                 # edges of et_row's map and of the 32-bit words
SPECIALS = [0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40]
ONE_HOT_ROW, ONE_HOT_K = 9, 77                            # W2[9] has ONE entry (at 77) and b2[9] = 0: H[9] = act(w A1[77])
ONE_HOT_COL, ONE_HOT_R = 40, 21                           # W2[:, 40] has ONE entry (at 21): dA1[40] = mA w dH[21]
ZERO_B_ROWS = [2, 64, ONE_HOT_ROW]                        # b2 = 0 there: H is exactly +0 in the all-zero column of A1
DYN = 2.0 ** -20
FULL = 1.0 + 2.0 ** -9 + 2.0 ** -17 - 2.0 ** -23           # bf16 parts 1, 2^-9 and 2^-17 - 2^-23: a dropped third part costs 2^-17 = 128 UNIT[3]


def plant_columns(N):
    """first and last column of a chunk, the last valid column of the ragged chunk and the first of that chunk"""
    return sorted(c for c in {0, 31, 32, 63, N - 1, 32 * ((N - 1) // 32)} if 0 <= c < N)


def zero_column(N):
    return N // 2 if N >= 3 and N // 2 not in plant_columns(N) else None


@functools.lru_cache(maxsize=None)
def weights(nh, dyn=False):
    """-> W2, b2, Wh, bh.  dyn: a row of W2 and a head row 2^-20 below the rest."""
    W2, b2 = rnd(C, C, seed=1, scale=C ** -0.5), rnd(C, seed=2)
    Wh, bh = rnd(nh, C, seed=3 + nh, scale=C ** -0.5), rnd(nh, seed=4 + nh)
    W2[ONE_HOT_ROW] = 0.0
    W2[:, ONE_HOT_COL] = 0.0
    W2[ONE_HOT_ROW, ONE_HOT_K], W2[ONE_HOT_R, ONE_HOT_COL] = 0.37, -0.53
    b2[ZERO_B_ROWS] = 0.0
    Wh[:, ONE_HOT_R] = 1.0                                 # ... and with nh = 1 and all bits set, dH[21] = dheads[0] exactly
    if dyn:
        W2[5] *= DYN
        b2[5] *= DYN
        Wh[nh - 1] *= DYN
        bh[nh - 1] *= DYN
    return W2, b2, Wh, bh


def wgrad_wh(nh, dyn=False):
    """Wh of the x6 weight-gradient cases: column 21 is 4, so the row-sum factor of that row's h3 scale (max |dheads| * sum_h
    |Wh[h][row]|) is 4 nh -- left out, the row overflows fp16; every other row's factor is below 1"""
    Wh = weights(nh, dyn)[2].clone()
    Wh[:, ONE_HOT_R] = 4.0
    return Wh


@functools.lru_cache(maxsize=16)
def a1_case(N, scale=1.0, dyn=False):
    """A1 [128][N] with SPECIALS at plant_columns() x (PLANT_ROWS + the one-hot channel) and an all-zero column"""
    A1 = rnd(C, N, seed=5 + N % 1000) * scale
    A1[ONE_HOT_K] = FULL * scale * (1 - 2 * (torch.arange(N) % 2)) * 2.0 ** (torch.arange(N) % 5)
    for ic, c in enumerate(plant_columns(N)):
        for ir, r in enumerate(PLANT_ROWS + [ONE_HOT_K]):
            A1[r, c] = SPECIALS[(ir + ic) % len(SPECIALS)]
    if zero_column(N) is not None:
        A1[:, zero_column(N)] = 0.0
    if dyn:
        A1[41] *= DYN
    return A1


def special_chunks(N, cus=None):
    """{chunk: factor} of dheads: one aligned chunk exactly zero, one x 2^-20, one x 2^20; with cus: more of them among the chunks
    the waves run SECOND and THIRD (index >= 8 cus, >= 16 cus)"""
    nchunks = (N + 31) // 32
    sp = {1: 0.0, 2: 2.0 ** -20, 3: 2.0 ** 20} if nchunks >= 5 else {}
    if cus is not None:
        sp.update({8 * cus + 1: 2.0 ** 20, 8 * cus + 2: 0.0})
        if nchunks > 16 * cus + 2:
            sp.update({16 * cus + 1: 2.0 ** -20, 16 * cus + 2: 2.0 ** 20})
    return sp


@functools.lru_cache(maxsize=16)
def dheads_case(nh, N, cus=None, plain=False):
    d = rnd(nh, N, seed=6 + nh + N % 1000)
    d[0] = FULL * (1 - 2 * (torch.arange(N) % 2)) * 2.0 ** (torch.arange(N) % 3)
    if not plain:
        for ch, f in special_chunks(N, cus).items():
            d[:, 32 * ch:32 * ch + 32] *= f
    return d


def x6_fwd_cases():
    """(N, nh, act, b2 given): every N with nh = 1 .. 7 in turn; every nh at N = 33 with the three activations and b2 = NULL"""
    return ([(N, 1 + i % 7, 1, True) for i, N in enumerate(NS_SMALL)] +
            [(33, nh, nh % 3, nh % 2 == 0) for nh in range(1, 8)] + [(257, 4, 1, False), (257, 6, 2, True), (255, 7, 0, False)])


def x6_dgrad_cases():
    """(N, nh, pattern of both sign words)"""
    return ([(N, 1 + (i + 3) % 7, BIT_PATTERNS[i % 5]) for i, N in enumerate(NS_SMALL)] +
            [(257, 7, p) for p in BIT_PATTERNS] + [(33, nh, 'random') for nh in range(1, 8)])


H3_FWD_VARIANTS = [(1.0, 1.0, False), (1.0, 64.0, False), (1.0, 1.0, True), (1e-5, 1.0, False), (1e3, 64.0, False)]   # (scale, amax slack, dyn)


def h3_fwd_variants():
    """(scale of A1, slack of amax_a1, dyn, act) at N = 257, nh = 7.  tanh at 1e3 is left out: it saturates, and every arithmetic
    then differs where a pre-activation of size 1 is a difference of terms of size 1e3 (test_hip_primitives.py::test_enc_tail_x6)."""
    return [(s, k, d, act) for s, k, d in H3_FWD_VARIANTS for act in (1, 0, 2) if not (act == 2 and s == 1e3)]

WIDE_FWD_NH = [1, 4, 7, 8, 9, 32, 33, 64, 65, 96, 97, 127, 128]
WIDE_DGRAD_NH = [1, 7, 8, 9, 12, 15, 16, 17, 31, 113, 128]


def wide_fwd_cases():
    """(N, nh, act, b2 given)"""
    return ([(257, nh, (1, 1, 2, 0)[i % 4], i % 5 != 3) for i, nh in enumerate(WIDE_FWD_NH)] +
            [(N, (23, 103)[i % 2], 1, True) for i, N in enumerate(NS_SMALL[:-1])])


def wide_dgrad_cases():
    """(N, nh, pattern, amax slack)"""
    return ([(257, nh, BIT_PATTERNS[i % 5], (1.0, 64.0)[i % 2]) for i, nh in enumerate(WIDE_DGRAD_NH)] +
            [(N, (12, 103)[i % 2], 'random', 1.0) for i, N in enumerate(NS_SMALL[:-1])])


def wgrad_chunks(cus):
    """one workgroup | two, three single-chunk workgroups | two chunks each, a last busy workgroup with ONE (the clamped DMA) and
    workgroups without any | three each (odd: the cell set parity ends on 0) | four each, the last busy one with two"""
    return [1, 2, 3, cus + 1, 2 * cus + 1, 3 * cus + 2]


WGRAD_X6_NH = [1, 4, 7]
WGRAD_WIDE_ROWS = [1, 7, 8, 31, 32, 33, 103, 128]
WGRAD_PADS = [0, 4, 64]


@functools.lru_cache(maxsize=8)
def wgrad_case(N, dyn=False):
    """-> A [128][N], D [128][N] (the wide kernel takes its first rows_d rows)"""
    A, D = rnd(C, N, seed=7 + N % 1000), rnd(C, N, seed=8 + N % 1000)
    A[ONE_HOT_K] = 0.0
    A[ONE_HOT_K, 5] = FULL                                  # column 77 of dW has ONE term per row
    if dyn:
        A[41] *= DYN
        D[1] *= DYN
    return A, D
