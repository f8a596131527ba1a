"""float64 restatement of the decoder's two-valued data gradient from stored sign bits (tvae_linear_dgrad_x6 with vg_bits,
include/tvae_hip.h; a plain helper module without GPU code, used by test_dense_bits_ref_cpu.py, test_dense_dgrad_bits_gpu.py
and test_dense_wgrad_step32_gpu.py).  Names as in the header:

  H [M][N]   the layer whose sign bits are stored: bit (n & 31) of word n >> 5 of row m is [H[m][n] > 0]
  W [M][K]   that layer's weight, dX [K][N] the gradient of its input, wo [M] the single-output Linear behind it, gy [N]
  a[m][n]    = 1 where the bit is set, else slope                          (LeakyReLU'(H))
  dX[k][n]   = mask[k][n] (add[k][n] + gy[n] sum_m wo[m] W[m][k] a[m][n])
  mask       = LeakyReLU' of aux, or of the recomputed first layer pre[k][n] = wc[k] . x'[n] + bc[k] + lb[n / Np][k], or 1
  gxr[n][c]  = sum_k wc[k][c] dX[k][n]                                      (fused first-layer backward)
  part[t][k] = sum_{n in the 128-column panel t} dX[k][n] (1, x'_0[n], x'_1[n]);  Simg, dbc, dWc: tvae_dec_in_total's totals
  g0[m]      = sum_n gy[n] a[m][n];  rs_db[m] = wo[m] g0[m];  rs_dwo[m] = rowdot[m] + bias[m] g0[m]
  csum[k]    = sum_m wo[m] W[m][k]                                          (rowsum of the scaled split)

Everything is torch.float64 on the CPU; arguments may come in any float dtype."""
import torch

SLOPE = 0.01
PANEL = 128                # columns per tile of the data gradient = per panel of the fused first-layer backward


def _F64(v):
    return torch.tensor(v, dtype=torch.float64)          # (a Python scalar in torch.where would make the result float32)


# ---- sign-bit words ---------------------------------------------------------------------------------------------------------
def unpack(words):
    """int32 [rows][N / 32] -> bool [rows][N]: column n is bit (n & 31) of word n >> 5."""
    w = words.to(torch.int64)
    return ((w[:, :, None] >> torch.arange(32)) & 1).reshape(w.shape[0], -1).bool()


def pack(mask):
    """bool [rows][N] (N % 32 == 0) -> int32 [rows][N / 32], the inverse of unpack."""
    b = mask.to(torch.int64).view(mask.shape[0], -1, 32)
    w = (b << torch.arange(32)).sum(-1)
    return (w - ((w >> 31) << 32)).to(torch.int32).contiguous()


def random_bits(rows, N, seed):
    """[rows][N / 32] random int32 words and the 0 / 1 matrix they encode (bit n & 31 of word n >> 5 is column n)."""
    g = torch.Generator().manual_seed(seed)
    words = torch.randint(-2 ** 31, 2 ** 31, (rows, N // 32), generator=g, dtype=torch.int64).to(torch.int32)
    return words, unpack(words)


# ---- the operation ----------------------------------------------------------------------------------------------------------
def act_factor(bits, slope=SLOPE):
    """a[m][n] = 1 where the bit is set, else slope."""
    return torch.where(bits, _F64(1.0), _F64(slope))


def first_layer_pre(xr, wc, bc, lb, Np):
    """pre[k][n] = wc[k] . x'[n] + bc[k] + lb[n // Np][k]  (bc / lb = None: 0); xr [N][2], wc [K][2], lb [N / Np][K]."""
    pre = wc.double() @ xr.double().t()
    if bc is not None:
        pre = pre + bc.double()[:, None]
    if lb is not None:
        pre = pre + lb.double()[torch.arange(xr.shape[0]) // Np].t()
    return pre


def lrelu_mask(v, slope=SLOPE):
    """v > 0 ? 1 : slope  (zeros of either sign, and everything below, take the slope)."""
    return torch.where(v > 0, _F64(1.0), _F64(slope))


def csum(W, wo):
    return (wo.double()[:, None] * W.double()).sum(0)


def dgrad(W, wo, gy, a, mask=None, add=None):
    """dX [K][N] from W [M][K], wo [M], gy [N], a [M][N] (act_factor), mask [K][N] or None (1), add [K][N] or None."""
    dX = (W.double() * wo.double()[:, None]).t() @ a.double() * gy.double()[None, :]
    if add is not None:
        dX = dX + add.double()
    return dX if mask is None else mask.double() * dX


def in_tail(dX, xr, wc, Np, panel=PANEL):
    """The fused backward of the first layer on dX [K][N]: (gxr [N][2], part [N / panel][K][3], Simg [N / Np][K], dbc [K],
    dWc [K][2]).  Np % panel == 0 (the launch has panel = 128; a smaller one serves small checks of this module)."""
    K, N = dX.shape
    assert Np % panel == 0 and N % Np == 0
    x = xr.double()
    gxr = dX.t() @ wc.double()
    cols = torch.stack([torch.ones(N, dtype=torch.float64), x[:, 0], x[:, 1]], 1)              # [N][3]
    part = torch.einsum('ktp,tpj->tkj', dX.view(K, N // panel, panel), cols.view(N // panel, panel, 3))
    Simg = part[:, :, 0].reshape(N // Np, Np // panel, K).sum(1)
    return gxr, part, Simg, part[:, :, 0].sum(0), part[:, :, 1:].sum(0)


def row_sums(a, gy, wo, rowdot, bias=None):
    """(g0, rs_db, rs_dwo), each [M]."""
    g0 = a.double() @ gy.double()
    b = torch.zeros_like(g0) if bias is None else bias.double()
    return g0, wo.double() * g0, rowdot.double() + b * g0


def tile_sums(bits, gy, panel=PANEL):
    """The per-tile partial sums the launch leaves in the first word of rs_part: [M][N / panel], sum over the tile of gy[n] [bit]."""
    return (bits.double() * gy.double()[None, :]).view(bits.shape[0], -1, panel).sum(2)
