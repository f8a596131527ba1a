"""torch.autograd.Function wrappers over the libtvae_hip.so C ABI (include/tvae_hip.h).

Internal activation layout is feature-major: [feature][image*positions + position].  Each Function
mirrors one stage of the reference hot path and cites the reference lines it replaces.  All compute
happens in the HIP library on the current torch stream; torch only provides device memory.
"""
from __future__ import annotations

import functools
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import tables
from ._lib import arithmetic, call, get_gemm_mode, parts, query, split_pipe

ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
LRELU_SLOPE = 0.01


def _expect(cond: bool, what: str) -> None:
    """Operand shapes are validated on the host before any launch: a kernel must never see a buffer smaller than
    its grid assumes (an out-of-bounds access can reset the GPU)."""
    if not cond:
        raise ValueError('tvae.ops: ' + what)


def act_code(activation) -> int:
    """Map an nn activation class/instance (reference ctor argument `activation`) to the kernel code."""
    import torch.nn as nn
    a = activation() if isinstance(activation, type) else activation
    if isinstance(a, nn.LeakyReLU):
        if abs(a.negative_slope - LRELU_SLOPE) > 0:
            raise NotImplementedError('only the default LeakyReLU slope 0.01 is built')
        return ACT_LRELU
    if isinstance(a, nn.Tanh):
        return ACT_TANH
    raise NotImplementedError(f'activation {type(a).__name__} has no HIP kernel (reference CLI: tanh | leakyrelu)')


# ---------------------------------------------------------------------------------------------
# optional in-run kernel timing (bench.py): events are recorded on the stream the kernels are launched on
# ---------------------------------------------------------------------------------------------
KERNEL_EVENTS = None     # set to {} to record (start, end) torch.cuda.Event pairs per entry point
# set to {} to record, per split-pipe entry point, (parts, MFMAs per product block) of EVERY launch as it was actually
# issued (not as the mode would suggest): bench.py derives its executed-FLOP figures from it, the tests assert on it
PARTS_LOG = None


def mfma_per_block(nparts: int, two_valued: bool = False) -> int:
    """Matrix instructions per 32x32x16 product block of a split-pipe launch: 6 (three bf16 parts), 3 (two fp16 parts, h3),
    1 (bf16); against the exact 0 / 1 operand of the two-valued gradient only the other operand's parts count (3 / 2 / 1)."""
    return {3: 3 if two_valued else 6, 2: 2 if two_valued else 3, 1: 1}[nparts]


class _timed:
    def __init__(self, name, nparts=None, two_valued=False):
        self.name = name
        self.nparts = nparts
        self.products = mfma_per_block(nparts, two_valued) if nparts is not None else None

    def __enter__(self):
        if PARTS_LOG is not None and self.nparts is not None:
            PARTS_LOG.setdefault(self.name, []).append((self.nparts, self.products))
        if KERNEL_EVENTS is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if KERNEL_EVENTS is not None:
            self.e.record()
            KERNEL_EVENTS.setdefault(self.name, []).append((self.s, self.e, self.products))
        return False


def _in_forward_arithmetic(backward):
    """Run an autograd backward in the arithmetic its forward ran in (`ctx.arith`): the fused branches a forward takes
    decide what it saves, so the backward must route the same way even when it executes outside the caller's
    `arithmetic(...)` block."""
    def wrapped(ctx, *grads):
        with arithmetic(ctx.arith):
            return backward(ctx, *grads)
    wrapped.__doc__ = backward.__doc__
    return wrapped


PATH_LOG = None          # set to a set() to record which fused branches a step actually took (tests assert on it)

# Inference-mode forward (reference: eval_model runs under torch.no_grad(), train_mnist.py:352-387; get_latent,
# clustering_mnist.py:121-161).  Inside torch.autograd.Function.forward grad mode is ALWAYS off, so the decision is taken by
# the caller (`needs_grad` over the op's differentiable inputs, src/models.py) and handed down through this switch: the
# forward then writes nothing that only a backward would read -- no conv2 activation H (1.14 GB at 64x64 / 256), no sign
# words, no decoder sign bits, no retained spectra -- and saves nothing on ctx.
_INFER = False


def needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class inference:
    """`with ops.inference(flag):` -- the Functions applied inside run their inference-mode forward when `flag`."""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        global _INFER
        self.prev, _INFER = _INFER, self.on
        return self

    def __exit__(self, *exc):
        global _INFER
        _INFER = self.prev
        return False


def _note(name: str) -> None:
    if PATH_LOG is not None:
        PATH_LOG.add(name)


def kernel_event_ms():
    """Mean milliseconds per launch for every recorded entry point (call after torch.cuda.synchronize())."""
    out = {}
    for k, v in (KERNEL_EVENTS or {}).items():
        ts = [s.elapsed_time(e) for s, e, _ in v]
        pr = [p_ for _, _, p_ in v if p_ is not None]
        out[k] = dict(launches=len(ts), mean_ms=sum(ts) / max(len(ts), 1), total_ms=sum(ts),
                      # MFMAs per product block as launched: time-weighted mean (all launches of an entry do the same
                      # algorithmic work in the bench) and the distinct values seen
                      mfma_per_block=(sum(p_ * t for (_, _, p_), t in zip(v, ts) if p_ is not None) /
                                      max(sum(t for (_, _, p_), t in zip(v, ts) if p_ is not None), 1e-30)) if pr else None,
                      mfma_per_block_seen=sorted(set(pr)))
    return out


# ---------------------------------------------------------------------------------------------
# workspaces and device tables (cached per device)
# ---------------------------------------------------------------------------------------------
_WS = {}
_TABLES = {}
# Buffers a captured hipGraph holds raw pointers to (tvae/graph.py calls pin_scratch() after capture).  Growing a scratch
# buffer REPLACES its tensor; without this list the old block would go back to the caching allocator while the graph still
# writes into it on every replay (a later, larger eager batch -- an uneven shard, a test set larger than the captured
# minibatch -- would trigger exactly that: ADVICE r03).  Once pinned, outgrown buffers are kept alive instead of freed: the
# graph keeps its blocks, eager calls get the new, larger ones.
_PINNED = {}             # pin token -> outgrown buffers kept alive for that graph


def pin_scratch() -> int:
    """Called after a capture: returns a token; until `unpin_scratch(token)` every scratch buffer that is outgrown is kept
    alive (the graph holds raw pointers into the blocks that existed at capture time)."""
    tok = (max(_PINNED) + 1) if _PINNED else 1
    _PINNED[tok] = []
    return tok


def unpin_scratch(token: int) -> None:
    _PINNED.pop(token, None)


def _replace_ws(key, new):
    old = _WS.get(key)
    if old is not None:
        for lst in _PINNED.values():
            lst.append(old)
    _WS[key] = new


# debugging aid (TVAE_POISON_WS=1; off by default, costs a fill per call): every workspace view handed out, and every named
# scratch buffer when it is (re)allocated, is filled with NaN first -- a kernel that reads what no kernel of the same call
# wrote then shows up as NaN instead of depending on what an earlier, larger problem left there
POISON_WS = os.environ.get('TVAE_POISON_WS', '0') == '1'


def workspace(device, floats: int) -> torch.Tensor:
    """Split-K scratch (grown on demand, reused across calls on the same stream).  The caller gets a view of EXACTLY the
    size it asked for: several entry points cap their number of reduction slices by the workspace they are handed, so
    passing "whatever the shared buffer has grown to" would make the summation order of a step depend on which other call
    had run before it (the first step of a process differed from every later one by 2e-7 on one tensor: round 3)."""
    key = (device.type, device.index)
    t = _WS.get(key)
    if t is None or t.numel() < floats:
        t = torch.empty(int(floats), dtype=torch.float32, device=device)
        _replace_ws(key, t)
    if POISON_WS:
        t[:int(floats)].fill_(float('nan'))
    return t[:int(floats)]


def _dev_table(key, device, builder):
    k = (key, device.type, device.index)
    t = _TABLES.get(k)
    if t is None:
        t = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in builder())
        _TABLES[k] = t
    return t


def tap_tables(k: int, R: int, device):
    return _dev_table(('taps', k, R), device, lambda: tables.rotation_taps(k, R))


def tap_tables_csr(k: int, R: int, device):
    return _dev_table(('csr', k, R), device, lambda: tables.rotation_taps_csr(k, R))


SKINNY_MAX = 8          # head projections with <= 8 output rows use the streaming kernels, wider ones the MFMA GEMM


def _seglen(N: int) -> int:
    # (a multiple of 4: every segment of a 16-byte aligned row then starts 16-byte aligned -- the float4 path of rowdot_seg)
    return max(2048, ((N + 255) // 256 + 3) // 4 * 4)


def _rowsum(X: torch.Tensor, M: int, N: int, out: Optional[torch.Tensor] = None, amax: Optional[torch.Tensor] = None,
            ld: int = 0) -> torch.Tensor:
    """out[m] = sum_n X[m][n] (deterministic two-level reduction).  amax (a zeroed device word): also receives max |X|.
    ld: floats between rows of X (0 = N)."""
    sl = _seglen(N)
    nseg = (N + sl - 1) // sl
    tmp = torch.empty(nseg, M, dtype=torch.float32, device=X.device)
    call('tvae_rowdot_seg', X, ld or N, None, 1, M, N, sl, tmp, amax)
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=X.device)
    call('tvae_seg_sum', tmp, nseg, M, out, 1.0, 0)
    return out


def _dense_x6_ok(rows: int, N: int) -> bool:
    """Dense layers on the split bf16 pipe: wide layers only (the 512-row tile would waste a 128-row layer)."""
    return split_pipe() and N % 128 == 0 and rows >= 256


def _p3() -> int:
    """parts for an entry point / operand form WITHOUT an h3 instance: the h3 mode runs those in the exact x6 arithmetic."""
    p = parts()
    return 3 if p == 2 else p


def _inf_norm(t: torch.Tensor) -> torch.Tensor:
    """max |t| as a one-element device tensor (one reduction launch, no temporary, no host synchronisation): the h3 scale
    word of an operand that is streamed from memory (include/tvae_hip.h: x_amax)."""
    return torch.linalg.vector_norm(t.reshape(-1), float('inf')).reshape(1)


def _split_weight(W: torch.Tensor, rows: int, K: int, transpose: bool, key: str, scale=None, nparts: int = 3):
    """W (out, in) -> fragment-ready cells for A(row, k) = W[row][k] (forward) or W[k][row] (dgrad): 3 x bf16 parts, or
    (nparts = 2) the 2 x fp16 parts of the h3 arithmetic.
    scale (K floats): A(row, k) *= scale[k] before the split; then also returns the row sums of the scaled operand
    (the two-valued implicit-gradient form of tvae_linear_dgrad_x6, include/tvae_hip.h)."""
    W = W.contiguous()
    w3 = _scratch(W.device, key, query('tvae_dense_x6_bytes', rows, K) // 4)
    csum = torch.empty(rows, dtype=torch.float32, device=W.device) if scale is not None else None
    call('tvae_dense_split2h' if nparts == 2 else 'tvae_dense_split3', W, W.shape[1], w3, w3.numel() * 4, rows, K,
         1 if transpose else 0, scale, csum)
    return w3 if scale is None else (w3, csum)


def _wgrad(dpre, X, M, N, K, virt=None, va=None, act=0, bits=None, rowdot_w=None, a_amax=None, x_amax=None, ld=0,
           nparts=None, x_amax_rows=False, two_val=False):
    """dW = dpre . X^T.  virt = dict(vg_wo, vg_gy, vg_act): dpre is the saved activation H, the gradient wo[m]*gy[n]*act'(H) is formed
    on the fly; va = dict(va_xr, va_wc, va_bc, va_lb, va_np): X is the coordinate layer's output act(..), recomputed (split pipe only).
    bits: [H > 0] as stored sign bits (dpre may then be None).  rowdot_w = the layer's own weight [M][K]: also returns
    rowdot[m] = sum_k W[m][k] dW[m][k] / wo[m] (taken before the multiplication), as (dW, rowdot).
    The arithmetic is the caller's: nparts of the split-pipe launch (None: _p3()), two_val = the two-valued form of the
    implicit LeakyReLU gradient (then with `bits`).  Two parts (h3) take the bounds of what is streamed from memory: the
    two-valued form x_amax unless X is recomputed (va), two plain operands a_amax and x_amax; x_amax_rows = x_amax holds one
    bound per row of X, not a single word."""
    dev_ = (dpre if dpre is not None else (X if X is not None else virt['vg_wo'])).device
    dW = torch.empty(M, K, dtype=torch.float32, device=dev_)
    need = 64 * max(M, 128) * max(K, 128)
    if split_pipe() and M >= 256 and K >= 128 and N % 16 == 0 and N >= 32:
        p = _p3() if nparts is None else nparts
        _expect(p != 2 or (two_val and bits is not None and (va is not None or x_amax is not None)) or
                (virt is None and va is None and a_amax is not None and x_amax is not None),
                'two-part weight gradient without the bounds of its streamed operands')
        ws = workspace(dev_, max(query('tvae_linear_wgrad_x6_ws_floats', M, N, K), 1 << 24))
        rowdot = torch.empty(M, dtype=torch.float32, device=dev_) if rowdot_w is not None else None
        with _timed('tvae_linear_wgrad_x6', p, two_val):
            call('tvae_linear_wgrad_x6', dpre, X, dW, ws, ws.numel(), M, N, K, ld or N, ld or N, 0,
                 **(virt or dict(vg_act=act)), vg_slope=LRELU_SLOPE, **(va or {}), vg_bits=bits, parts=p,
                 rd_w=rowdot_w.contiguous() if rowdot_w is not None else None, rd_ldw=K, rd_rowdot=rowdot, a_amax=a_amax,
                 x_amax=x_amax, x_amax_rows=int(x_amax_rows))
        return dW if rowdot_w is None else (dW, rowdot)
    _expect(virt is None and va is None and rowdot_w is None, 'implicit operands need the split-pipe weight gradient')
    ws = workspace(dev_, max(need, 1 << 24))
    call('tvae_linear_wgrad', dpre, X, dW, ws, ws.numel(), M, N, K, ld or N, ld or N, 0)
    return dW


# ---------------------------------------------------------------------------------------------
# rotated bank + lifting convolution
# ---------------------------------------------------------------------------------------------
def rotate_bank(weight: torch.Tensor, R: int) -> torch.Tensor:
    """GroupConv.trans_filter (src/models.py:174-197): (C,Cin,1,k,k) -> bank [C*R][Cin*k*k]."""
    C, Cin, D, k, _ = weight.shape
    if D != 1:
        raise NotImplementedError('input_rot_dim != 1 is never used by the reference (models.py:290,346)')
    idx, w = tap_tables(k, R, weight.device)
    bank = torch.empty(C * R, Cin * k * k, dtype=torch.float32, device=weight.device)
    call('tvae_rotate_bank_fwd', weight.contiguous(), idx, w, bank, C, Cin, k, R)
    return bank


def rotate_bank_bwd(dbank: torch.Tensor, C: int, Cin: int, k: int, R: int) -> torch.Tensor:
    ptr, er, ed, ew = tap_tables_csr(k, R, dbank.device)
    dW = torch.empty(C, Cin, 1, k, k, dtype=torch.float32, device=dbank.device)
    call('tvae_rotate_bank_bwd', dbank, ptr, er, ed, ew, dW, C, Cin, k, R, 0)
    return dW


def _use_x6(Cin, n, k, pad) -> bool:
    """Lifting convolution on the bf16 matrix pipe (exact 3 x bf16 operand split, six products; fp32-equivalent)."""
    return split_pipe() and bool(query('tvae_conv1_x6_supported', Cin, n, k, pad))


def _scratch(device, key, floats: int) -> torch.Tensor:
    """Named persistent scratch buffers (split operands of the x6 convolution)."""
    k_ = (key, device.type, device.index)
    t = _WS.get(k_)
    if t is None or t.numel() < floats:
        t = torch.empty(int(floats), dtype=torch.float32, device=device)
        if POISON_WS:
            t.fill_(float('nan'))
        _replace_ws(k_, t)
    return t


# Routing switches, each kept alive by a test: TVAE_CONV_DFT=0 -- the direct split-pipe convolution instead of the
# frequency-domain one (bench.py's conv_direct_form line; tests/test_hip_modules.py runs the direct kernels through
# geometries the DFT plan rejects); FUSE_ENC_TAIL = False -- the unfused encoder tail (test_encoder_tail_paths_agree); at the
# decoder, TVAE_DEC_PAD=0 -- no padding of 28 x 28 / 50 x 50 pixel ranges to the GEMM tile
# (test_decoder_pads_pixel_ranges_to_the_gemm_tile) and TVAE_DEC_LD_PAD (test_decoder_padded_row_stride_is_layout_only).
# Every other fusion of rounds 2-6 won its A/B (profiles/README.md has every measurement) and is unconditional; the unfused
# branches remain as the paths of shapes the fused kernels do not cover.
CONV_DFT = os.environ.get('TVAE_CONV_DFT', '1') != '0'
FUSE_ENC_TAIL = True


def _use_dft(B, Cin, n, k, pad, C, R) -> bool:
    """Frequency-domain lifting convolution (DFT along x + batched split-pipe GEMM): 13x fewer matrix FLOPs than the direct
    form; same arithmetic mode as 'x6' (TVAE_CONV_DFT=0 keeps the direct x6 kernels)."""
    return CONV_DFT and split_pipe() and bool(query('tvae_conv1_dft_supported', B, Cin, n, k, pad, C, R))


def conv1_forward(y, weight, bias, C, R, k, pad, act, bank=None):
    """Rotated bank + lifting convolution: returns (out, at), `at` being what the frequency-domain path keeps for the weight
    gradient (A^T, then max |out| per channel: conv1_out_max) and None on the other paths.  `bank`: a ready [C*R][Cin*k*k]
    bank (the plain convolution of --groupconv 0 is the R = 1 case with the weight itself as the bank)."""
    B, Cin, n, _ = y.shape
    Ho = n + 2 * pad - k + 1
    if bank is None:
        bank = rotate_bank(weight, R)
    out = torch.empty(C, B * R * Ho * Ho, dtype=torch.float32, device=y.device)
    if _use_dft(B, Cin, n, k, pad, C, R):
        # (the columns that pad (image, row) to a multiple of 128 are zeroed by the entry point when there are any)
        at = torch.empty(query('tvae_conv1_dft_at_floats', B, Cin, n, k, pad, C, R), dtype=torch.float32,
                         device=y.device)
        ws = _scratch(y.device, 'dft_ws', query('tvae_conv1_dft_ws_floats', B, Cin, n, k, pad, C, R))
        _note('conv1.dft')
        if query('tvae_conv1_dft_ring', B, Cin, n, k, pad, C, R):
            _note('conv1.dft_ring')      # ring (LDS-DMA) transforms along w: abi_conv_dft.hip dft_plan
        with _timed('tvae_conv1_fwd', parts()):
            call('tvae_conv1_fwd_dft', y, bank, bias, out, at, ws, ws.numel(), B, Cin, n, k, pad, C, R, act,
                 LRELU_SLOPE, parts())
        return out, at
    if _use_x6(Cin, n, k, pad):
        a3 = _scratch(y.device, 'x6_bank', query('tvae_conv1_x6_bank_bytes', C, R, Cin, k) // 4)
        call('tvae_bank_split3', bank, a3, a3.numel() * 4, C, R, Cin, k)
        _note('conv1.x6')
        with _timed('tvae_conv1_fwd', 3):
            call('tvae_conv1_fwd_x6', y, a3, bias, out, B, Cin, n, k, pad, C, R, act, LRELU_SLOPE)
        return out, None
    _note('conv1.f32')
    with _timed('tvae_conv1_fwd'):
        call('tvae_conv1_fwd', y, bank, bias, out, B, Cin, n, k, pad, C, R, act, LRELU_SLOPE)
    return out, None


def conv1_out_max(at: torch.Tensor, C: int) -> torch.Tensor:
    """max |out| per channel, left behind A^T by the output transform of the frequency-domain convolution (a view of `at`):
    the h3 scales of the encoder tail."""
    return at[-C:]


def conv1_wgrad(y, dpre, C, R, k, pad, at=None, dbias=None):
    """Weight gradient of the lifting convolution: returns dbank.  With the frequency-domain path (`at` from the forward
    call) the bias gradient is a by-product: pass `dbias` (C floats) to receive it."""
    B, Cin, n, _ = y.shape
    dbank = torch.empty(C * R, Cin * k * k, dtype=torch.float32, device=y.device)
    if at is not None:
        wsd = _scratch(y.device, 'dft_ws', query('tvae_conv1_dft_ws_floats', B, Cin, n, k, pad, C, R))
        with _timed('tvae_conv1_wgrad', parts()):
            call('tvae_conv1_wgrad_dft', dpre, at, dbank, dbias, wsd, wsd.numel(), B, Cin, n, k, pad, C, R, parts())
        return dbank
    ws = workspace(y.device, max(1 << 24, 16 * dbank.numel()))
    if _use_x6(Cin, n, k, pad):
        d3 = _scratch(y.device, 'x6_dy', query('tvae_conv1_x6_dy_bytes', B, C, R, n, k, pad) // 4)
        call('tvae_dy_split3', dpre, d3, d3.numel() * 4, B, Cin, n, k, pad, C, R)
        with _timed('tvae_conv1_wgrad', 3):
            call('tvae_conv1_wgrad_x6', y, d3, dbank, ws, ws.numel(), B, Cin, n, k, pad, C, R)
        return dbank
    with _timed('tvae_conv1_wgrad'):
        call('tvae_conv1_wgrad', y, dpre, dbank, ws, ws.numel(), B, Cin, n, k, pad, C, R)
    return dbank


def conv1_backward(y, dA1, C, R, k, pad, at):
    """(dbank, db1) of the lifting convolution from the gradient dA1 [C][N] of its pre-activation.  The bias gradient is a
    by-product of the frequency-domain weight gradient (`at` kept by the forward), a row sum of dA1 otherwise."""
    db1 = torch.empty(C, dtype=torch.float32, device=y.device) if at is not None else _rowsum(dA1, C, dA1.shape[1])
    return conv1_wgrad(y, dA1, C, R, k, pad, at, db1 if at is not None else None), db1


class BankFn(torch.autograd.Function):
    """GroupConv.trans_filter as a differentiable op: (C,Cin,1,k,k) -> [C*R][Cin*k*k]."""

    @staticmethod
    def forward(ctx, weight, R):
        ctx.cfg = (weight.shape[0], weight.shape[1], weight.shape[3], R)
        return rotate_bank(weight, R)

    @staticmethod
    def backward(ctx, g):
        C, Cin, k, R = ctx.cfg
        return rotate_bank_bwd(g.contiguous().view(C * R, Cin * k * k), C, Cin, k, R), None


class GroupConvFn(torch.autograd.Function):
    """GroupConv.forward (src/models.py:202-225) as one op: rotated bank + implicit-GEMM conv + bias.
    Returns the reference layout (B, C, R, Ho, Ho).  No input gradient (the input is data)."""

    @staticmethod
    def forward(ctx, y, weight, bias, R, pad):
        C, Cin, _, k, _ = weight.shape
        y = y.contiguous().view(y.shape[0], Cin, y.shape[-2], y.shape[-1])
        B, n = y.shape[0], y.shape[-1]
        Ho = n + 2 * pad - k + 1
        out, ctx.at = conv1_forward(y, weight, bias, C, R, k, pad, ACT_NONE)
        ctx.arith = get_gemm_mode()
        ctx.save_for_backward(y)
        ctx.cfg = (C, Cin, k, R, pad, B, Ho, bias is not None)
        return out.view(C, B, R, Ho, Ho).permute(1, 0, 2, 3, 4)

    @staticmethod
    @_in_forward_arithmetic
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        C, Cin, k, R, pad, B, Ho, has_bias = ctx.cfg
        if ctx.needs_input_grad[0]:
            raise NotImplementedError('GroupConv input gradient is not part of the hot path (input is data)')
        dpre = g.permute(1, 0, 2, 3, 4).contiguous().view(C, B * R * Ho * Ho)
        db = None                                        # (optional here, and summed after the bank: not conv1_backward)
        if has_bias and ctx.at is not None:
            db = torch.empty(C, dtype=torch.float32, device=y.device)
        dbank = conv1_wgrad(y, dpre, C, R, k, pad, ctx.at, db)
        dW = rotate_bank_bwd(dbank, C, Cin, k, R)
        if has_bias and db is None:
            db = _rowsum(dpre, C, dpre.shape[1])
        return None, dW, db, None, None


def _enc_tail_perm(device) -> torch.Tensor:
    """Column order of W2^T for tvae_enc_tail_dgrad_x6 (include/tvae_hip.h): slot 16 u + 8 h + j holds row
    16 u + 8 (j >> 2) + 4 h + (j & 3) -- the order in which the first GEMM's accumulator registers feed the second."""
    def build():
        s_ = np.arange(128)
        u, h, j = s_ // 16, (s_ % 16) // 8, s_ % 8
        return (16 * u + 8 * (j // 4) + 4 * h + (j % 4),)
    return _dev_table(('enc_tail_perm',), device, build)[0]


ENC_TAIL_FUSED_MAX_ROWS = 7      # head rows of tvae_enc_tail_*_x6 (enc_tail_x6_kernels.hpp)
ENC_TAIL_WIDE_MAX_ROWS = 128     # ... of tvae_enc_tail_*_wide, which take over at SKINNY_MAX (enc_tail_wide_kernels.hpp)
ENC_TAIL_MAX_COLS = 1 << 25      # the fused kernels index 32 rows with 32-bit byte offsets (abi_enc_tail_x6.hip: ET_MAX_LD)


class EncoderRoute(NamedTuple):
    """Every structural decision of EncoderFn's tail (conv2 + the stacked head projection), taken once by encoder_route()
    in the forward and kept on ctx: the backward routes by it, so the two passes cannot disagree about what was stored."""
    tail: str            # 'fused': conv2 + heads in one pass over A1 and one over H (tvae_enc_tail_*_x6); 'wide': as two chained
    #                      GEMMs per 32-column chunk, H handed over in registers (tvae_enc_tail_*_wide); 'plain': separate launches
    parts: int           # `parts` of the tail's forward launch (0: 'plain')
    h3: bool             # the tail launches take max |A1| per channel (left by the frequency-domain conv1) as their h3 scales
    bits: bool           # sign words of H and A1 are stored: the data gradient is the tail kernel's, from them alone
    wgrad: str           # 'x6': dW2 from A1, dheads and the sign words (tvae_enc_tail_wgrad_x6; dH is never written); 'wide': dWh
    #                      and dW2 as two tvae_enc_tail_wgrad_wide launches over stored operands; 'plain': the generic GEMMs
    infer: bool          # inference-mode forward: head rows only, nothing is kept for a backward


def encoder_route(C: int, C2: int, nh: int, N: int, act: int, out_max: bool, infer: bool) -> EncoderRoute:
    """The route of EncoderFn's tail for C -> C2 channels, nh head rows and N columns in the current arithmetic; out_max:
    conv1 took the frequency-domain path and left max |A1| per channel (conv1_out_max).  Pure: no tensor, no launch.
    The fused kernels are built for the reference's 128 channels on the split pipe and fewer than 2^25 columns (beyond that
    the plain path with 64-bit indexing takes over); the wide ones keep both weights in LDS, which the exact three-part
    split does not fit: h3 (needs the bounds of A1) or bf16 arithmetic."""
    p = parts()
    tail = 'plain'
    if FUSE_ENC_TAIL and split_pipe() and C == 128 and C2 == 128 and N < ENC_TAIL_MAX_COLS:
        if nh <= ENC_TAIL_FUSED_MAX_ROWS:
            tail = 'fused'
        elif SKINNY_MAX <= nh <= ENC_TAIL_WIDE_MAX_ROWS and (p == 1 or (p == 2 and out_max)):
            tail = 'wide'
    h3 = tail != 'plain' and p == 2 and out_max
    bits = tail != 'plain' and act == ACT_LRELU and not infer
    # the fused weight gradients reduce over 32-column chunks; the wide one exists in h3 only (bounds of both operands)
    wgrad = 'plain' if not (bits and N % 32 == 0) else 'x6' if tail == 'fused' else 'wide' if h3 else 'plain'
    return EncoderRoute(tail=tail, parts={'plain': 0, 'wide': p, 'fused': 2 if h3 else _p3()}[tail], h3=h3, bits=bits,
                        wgrad=wgrad, infer=infer)


def _heads_forward(Wh, bh, H, heads, nh, C2, N):
    """heads = Wh H + bh, the stacked head projection on its own: streaming kernel or GEMM (SKINNY_MAX)."""
    if nh <= SKINNY_MAX:
        call('tvae_heads_fwd', Wh.contiguous(), H, N, bh, heads, N, nh, C2, N)
    else:
        call('tvae_linear_fwd', Wh.contiguous(), H, bh, None, 1, None, heads, nh, N, C2, N, N, ACT_NONE, LRELU_SLOPE)


def _heads_backward(Wh, dheads, H, dH, nh, C2, N, act):
    """Backward of the head projection through the activation that produced H: returns (dWh, db2) and fills
    dH = act'(H) . Wh^T dheads.  dH = None (nh <= SKINNY_MAX only): the sums alone."""
    if nh <= SKINNY_MAX:
        # one pass over H: masked dgrad + dWh + the row sums of dH (= db2)
        npan = (N + 511) // 512
        part = workspace(H.device, npan * C2 * (nh + 1) + 4 + 64 * C2 * (nh + 1))      # + room for the two-stage total
        tot = torch.empty(nh + 1, C2, dtype=torch.float32, device=H.device)
        call('tvae_heads_bwd', Wh.contiguous(), dheads, N, H, N, dH, N, nh, C2, N, act, LRELU_SLOPE, part,
             part.numel(), tot)
        return tot[:nh], tot[nh]
    dWh = _wgrad(dheads, H, nh, N, C2)
    call('tvae_linear_dgrad', Wh.contiguous(), dheads, None, H, dH, nh, N, C2, N, N, act, LRELU_SLOPE)
    return dWh, _rowsum(dH, C2, N)


class EncoderFn(torch.autograd.Function):
    """conv1 -> act -> conv2 (1x1x1) -> act -> {conv_a, conv_r, conv_z} (src/models.py:354-358,390-392).

    Output: heads [3+2*zd][B*R*Ho*Ho] feature-major, rows = (logit, theta_mu, theta_logstd, z_mu.., z_logstd..).
    Backward fuses every activation derivative into the producing dgrad epilogue."""

    @staticmethod
    def forward(ctx, y, w1, b1, W2, b2, Wh, bh, R, pad, act):
        C, Cin, _, k, _ = w1.shape
        _expect(y.numel() == y.shape[0] * Cin * y.shape[-1] * y.shape[-2] and y.shape[-1] == y.shape[-2],
                f'encoder input {tuple(y.shape)} is not (B, {Cin}, n, n)')
        y = y.contiguous().view(y.shape[0], Cin, y.shape[-2], y.shape[-1])
        B, n = y.shape[0], y.shape[-1]
        Ho = n + 2 * pad - k + 1
        _expect(Ho >= 1, f'kernel {k} with padding {pad} does not fit a {n}x{n} image')
        _expect(R in (4, 8, 16), f'groupconv must be 4, 8 or 16 (got {R})')
        N = B * R * Ho * Ho
        C2, nh = W2.shape[0], Wh.shape[0]
        _expect(tuple(W2.shape) == (C2, C) and tuple(Wh.shape) == (nh, C2) and b1.numel() == C and
                b2.numel() == C2 and bh.numel() == nh, 'encoder parameter shapes are inconsistent')
        A1, at = conv1_forward(y, w1, b1, C, R, k, pad, act)
        rt = encoder_route(C, C2, nh, N, act, at is not None, _INFER)
        # inference: the fused tails write the head rows only -- H is neither allocated nor stored (include/tvae_hip.h, ABI 6)
        H = None if (rt.infer and rt.tail != 'plain') else torch.empty(C2, N, dtype=torch.float32, device=y.device)
        heads = torch.empty(nh, N, dtype=torch.float32, device=y.device)
        a1max = conv1_out_max(at, C) if rt.h3 else None
        # sign words of H and A1: all the fused data gradient reads of them
        bits = torch.empty(2, N, 4, dtype=torch.int32, device=y.device) if rt.bits else (None, None)
        if rt.infer:
            _note('enc.inference')
        if rt.tail == 'plain':
            call('tvae_linear_fwd', W2.contiguous(), A1, b2, None, 1, None, H, C2, N, C, N, N, act, LRELU_SLOPE)
            _heads_forward(Wh, bh, H, heads, nh, C2, N)
        else:
            w3 = _split_weight(W2, C2, C, False, 'enc_w2', nparts=rt.parts)
            if rt.tail == 'wide':
                wh = _split_weight(Wh[:, _enc_tail_perm(y.device)], nh, C2, False, 'enc_whp', nparts=rt.parts)
                name, args = 'tvae_enc_tail_fwd_wide', (w3, wh, A1, N, b2, bh.contiguous())
            else:
                name, args = 'tvae_enc_tail_fwd_x6', (w3, A1, N, b2, Wh.contiguous(), bh.contiguous())
            _note('enc.tail_fwd_wide' if rt.tail == 'wide' else 'enc.tail_fwd_x6')
            with _timed(name, rt.parts):
                call(name, *args, nh, H, N, heads, N, bits[0], bits[1], C, N, act, LRELU_SLOPE, rt.parts, a1max)
        if rt.infer:
            return heads
        ctx.save_for_backward(y, W2, Wh, A1, H)
        ctx.route, ctx.at, ctx.bits = rt, at, bits
        ctx.a1max = a1max                                # (a view of `at`: the h3 scales of the weight gradients, too)
        # wide tail, h3: bound per row of H = act(W2 A1 + b2) for the weight gradient that streams H (|act(x)| <= |x|)
        ctx.hrows = torch.addmv(b2.detach().abs(), W2.detach().abs(), a1max) if (rt.tail == 'wide' and rt.h3) else None
        ctx.arith = get_gemm_mode()
        ctx.cfg = (C, Cin, k, R, pad, B, Ho, act)
        return heads

    @staticmethod
    @_in_forward_arithmetic
    def backward(ctx, dheads):
        y, W2, Wh, A1, H = ctx.saved_tensors
        C, Cin, k, R, pad, B, Ho, act = ctx.cfg
        rt = ctx.route
        N = B * R * Ho * Ho
        C2, nh = W2.shape[0], Wh.shape[0]
        dev = y.device
        dheads = dheads.contiguous()
        wide_bw = rt.tail == 'wide' and rt.bits
        # h3 bounds of the wide backward: max |dheads| (by the way of its row sums) and max |dH| (of those of dH)
        dmax, dhmax = torch.zeros(2, dtype=torch.float32, device=dev).split(1) if (wide_bw and rt.h3) else (None, None)
        dbh = _rowsum(dheads, nh, N, amax=dmax)
        # data gradient of the tail from the sign words (the dgrad launches have an h3 instance whatever the forward ran in)
        dH = None
        if wide_bw:
            # dH = act'(H) . Wh^T dheads and dA1 = act'(A1) . W2^T dH in one launch (dH handed over in registers and stored
            # once for the two weight gradients below)
            wht = _split_weight(Wh, C2, nh, True, 'enc_wht', nparts=parts())
            w3p = _split_weight(W2.t()[:, _enc_tail_perm(dev)], C, C2, False, 'enc_w2p', nparts=parts())
            dH = torch.empty(C2, N, dtype=torch.float32, device=dev)
            dA1 = torch.empty(C, N, dtype=torch.float32, device=dev)
            _note('enc.tail_dgrad_wide')
            with _timed('tvae_enc_tail_dgrad_wide', parts()):
                call('tvae_enc_tail_dgrad_wide', wht, w3p, dheads, N, nh, ctx.bits[0], ctx.bits[1], dH, N, dA1, N, C, N,
                     LRELU_SLOPE, parts(), dmax)
        elif rt.bits:
            # dA1 straight from the head gradients and the sign words (dH is formed in registers, never stored); h3
            # instance: 128 x 128 GEMM on two fp16 parts, scale per 32-column chunk
            w3p = _split_weight(W2.t()[:, _enc_tail_perm(dev)], C, C2, False, 'enc_w2p', nparts=parts())
            wh3 = _scratch(dev, 'enc_wh3', query('tvae_dense_x6_bytes', C2, nh) // 4)
            call('tvae_dense_split3', Wh.contiguous(), C2, wh3, wh3.numel() * 4, C2, nh, 1, None, None)
            dA1 = torch.empty(C, N, dtype=torch.float32, device=dev)
            _note('enc.tail_dgrad_x6')
            with _timed('tvae_enc_tail_dgrad_x6', parts()):
                call('tvae_enc_tail_dgrad_x6', w3p, wh3, dheads, N, nh, ctx.bits[0], ctx.bits[1], dA1, N, C, N,
                     LRELU_SLOPE, parts())
        # weight gradients of the head projection and of conv2
        if rt.wgrad == 'wide':
            # both as cooperative reductions over two stored operands (enc_tail_wgrad_plain_kernel)
            _note('enc.tail_wgrad_wide')
            wsw = _scratch(dev, 'enc_wgrad_slabs', query('tvae_enc_tail_wgrad_x6_ws_floats', N))
            dWf = torch.empty(2, C2, C, dtype=torch.float32, device=dev)
            with _timed('tvae_enc_tail_wgrad_wide', 2):
                call('tvae_enc_tail_wgrad_wide', dheads, N, nh, H, N, dWf[0], wsw, wsw.numel(), C2, N, dmax, ctx.hrows)
            db2 = _rowsum(dH, C2, N, amax=dhmax)
            with _timed('tvae_enc_tail_wgrad_wide', 2):
                call('tvae_enc_tail_wgrad_wide', dH, N, C2, A1, N, dWf[1], wsw, wsw.numel(), C, N, dhmax, ctx.a1max)
            dWh, dW2 = dWf[0, :nh], dWf[1]
        elif wide_bw:
            dWh, db2, dW2 = _wgrad(dheads, H, nh, N, C2), _rowsum(dH, C2, N), _wgrad(dH, A1, C2, N, C)
        elif rt.wgrad == 'x6':
            # conv2's in one pass from A1, the head gradients and the sign words of H (dH is formed inside the GEMM's operand
            # build and never written); dWh / db2 from a sums-only pass over H
            dWh, db2 = _heads_backward(Wh, dheads, H, None, nh, C2, N, act)
            _note('enc.tail_wgrad_x6')
            dW2 = torch.empty(C2, C, dtype=torch.float32, device=dev)
            wsw = _scratch(dev, 'enc_wgrad_slabs', query('tvae_enc_tail_wgrad_x6_ws_floats', N))
            with _timed('tvae_enc_tail_wgrad_x6', rt.parts):
                call('tvae_enc_tail_wgrad_x6', A1, N, dheads, N, nh, ctx.bits[0], Wh.contiguous(), dW2, wsw, wsw.numel(), C,
                     N, LRELU_SLOPE, rt.parts, ctx.a1max)
        else:
            dH = torch.empty(C2, N, dtype=torch.float32, device=dev)
            dWh, db2 = _heads_backward(Wh, dheads, H, dH, nh, C2, N, act)
            dW2 = _wgrad(dH, A1, C2, N, C)
        if not rt.bits:
            dA1 = torch.empty(C, N, dtype=torch.float32, device=dev)
            call('tvae_linear_dgrad', W2.contiguous(), dH, None, A1, dA1, C2, N, C, N, N, act, LRELU_SLOPE)
        del dH
        dbank, db1 = conv1_backward(y, dA1, C, R, k, pad, ctx.at)
        dw1 = rotate_bank_bwd(dbank, C, Cin, k, R)
        return None, dw1, db1, dW2, db2, dWh, dbh, None, None, None


class TransAttnEncoderFn(torch.autograd.Function):
    """Translation-attention encoder with pooled rotation (reference src/models.py:268-319) on the
    same kernels as the main encoder: conv1 (lifting convolution, or the plain R = 1 convolution of --groupconv 0) ->
    act -> fc_r rotation pooling (`tvae_rot_pool_*`) -> conv2 (1x1) -> act -> {conv_a, conv_r, conv_z} stacked.
    Output: heads [1 + 2 + 2*zd][B*Ho*Ho] feature-major."""

    @staticmethod
    def forward(ctx, y, w1, b1, fw, fb, W2, b2, Wh, bh, R, pad, act):
        C = w1.shape[0]
        plain = w1.dim() == 4                            # nn.Conv2d weight (C, Cin, k, k): groupconv = 0
        Cin, k = w1.shape[1], w1.shape[-1]
        y = y.contiguous().view(y.shape[0], Cin, y.shape[-2], y.shape[-1])
        B, n = y.shape[0], y.shape[-1]
        Ho = n + 2 * pad - k + 1
        _expect(Ho >= 1 and (plain or R in (4, 8, 16)), 'translation-attention encoder geometry')
        Re = 1 if plain else R
        P = Ho * Ho
        A1, ctx.at = conv1_forward(y, None if plain else w1, b1, C, Re, k, pad, act,
                                   bank=w1.contiguous().view(C, Cin * k * k) if plain else None)
        _note('trans_attn.plain' if plain else 'trans_attn.rot_pool')
        if plain:
            X = A1                                       # [C][B*P]
        else:
            X = torch.empty(C, B * P, dtype=torch.float32, device=y.device)
            call('tvae_rot_pool_fwd', A1, fw.contiguous().view(-1), fb.contiguous(), X, C, B, R, P)
        N = B * P
        C2, nh = W2.shape[0], Wh.shape[0]
        H = torch.empty(C2, N, dtype=torch.float32, device=y.device)
        call('tvae_linear_fwd', W2.contiguous(), X, b2, None, 1, None, H, C2, N, C, N, N, act, LRELU_SLOPE)
        heads = torch.empty(nh, N, dtype=torch.float32, device=y.device)
        _heads_forward(Wh, bh, H, heads, nh, C2, N)
        ctx.save_for_backward(y, w1, fw, W2, Wh, A1, X, H)
        ctx.cfg = (C, Cin, k, R, pad, B, Ho, act, plain)
        ctx.arith = get_gemm_mode()
        return heads

    @staticmethod
    @_in_forward_arithmetic
    def backward(ctx, dheads):
        y, w1, fw, W2, Wh, A1, X, H = ctx.saved_tensors
        C, Cin, k, R, pad, B, Ho, act, plain = ctx.cfg
        P = Ho * Ho
        N = B * P
        C2, nh = W2.shape[0], Wh.shape[0]
        dev = y.device
        dheads = dheads.contiguous()
        dbh = _rowsum(dheads, nh, N)
        dH = torch.empty(C2, N, dtype=torch.float32, device=dev)
        dWh, db2 = _heads_backward(Wh, dheads, H, dH, nh, C2, N, act)
        dW2 = _wgrad(dH, X, C2, N, C)
        dX = torch.empty(C, N, dtype=torch.float32, device=dev)
        # the pooled tensor is not an activation output: plain data gradient (groupconv 0: X = act(conv1), masked)
        call('tvae_linear_dgrad', W2.contiguous(), dH, None, A1 if plain else None, dX, C2, N, C, N, N,
             act if plain else ACT_NONE, LRELU_SLOPE)
        dfw = dfb = None
        if plain:
            dA1 = dX
        else:
            dA1 = torch.empty_like(A1)
            nb = min(1024, (C * N + 255) // 256)
            partp = workspace(dev, (R + 1) * nb)
            dtot = torch.empty(R + 1, dtype=torch.float32, device=dev)
            call('tvae_rot_pool_bwd', A1, dX, fw.contiguous().view(-1), dA1, partp, partp.numel(), dtot, C, B, R, P, act,
                 LRELU_SLOPE)
            dfw, dfb = dtot[:R].view(1, R), dtot[R:]
        dbank, db1 = conv1_backward(y, dA1, C, 1 if plain else R, k, pad, ctx.at)
        dw1 = dbank.view(C, Cin, k, k) if plain else rotate_bank_bwd(dbank, C, Cin, k, R)
        return None, dw1, db1, dfw, dfb, dW2, db2, dWh, dbh, None, None, None


class MlpFn(torch.autograd.Function):
    """Linear / ResidLinear stack of the MLP encoder (reference src/models.py:229-260) on the GEMM kernels, feature-major:
    h0 = act(W0 x + b0); hi = act(Wi h + bi [+ h]); out = Wl h + bl.  x is data (no input gradient)."""

    @staticmethod
    def forward(ctx, x, act, resid, *params):
        nl = len(params) // 2
        _expect(nl >= 2 and len(resid) == nl and x.dim() == 2 and params[0].shape[1] == x.shape[1], 'MLP encoder shapes')
        B = x.shape[0]
        xt = x.t().contiguous()                          # [n][B]
        hs = [xt]
        for i in range(nl):
            W, b = params[2 * i], params[2 * i + 1]
            M, K = W.shape
            _expect(K == hs[-1].shape[0] and (not resid[i] or M == K), 'MLP encoder layer widths')
            h = torch.empty(M, B, dtype=torch.float32, device=x.device)
            call('tvae_linear_fwd', W.contiguous(), hs[-1], b, None, 1, hs[-1] if resid[i] else None, h, M, B, K, B, B,
                 act if i + 1 < nl else ACT_NONE, LRELU_SLOPE)
            hs.append(h)
        _note('mlp_encoder.kernels')
        ctx.save_for_backward(*hs[:-1], *params[0::2])
        ctx.cfg = (act, tuple(resid), nl, B)
        ctx.arith = get_gemm_mode()
        return hs[-1].t()

    @staticmethod
    @_in_forward_arithmetic
    def backward(ctx, dout):
        act, resid, nl, B = ctx.cfg
        hs, Ws = ctx.saved_tensors[:nl], ctx.saved_tensors[nl:]
        d = dout.t().contiguous()                        # gradient of layer i's pre-activation, [M][B]
        grads = [None] * (2 * nl)
        for i in range(nl - 1, -1, -1):
            M, K = Ws[i].shape
            grads[2 * i] = _wgrad(d, hs[i], M, B, K)
            grads[2 * i + 1] = _rowsum(d, M, B)
            if i > 0:
                dprev = torch.empty(K, B, dtype=torch.float32, device=d.device)
                call('tvae_linear_dgrad', Ws[i].contiguous(), d, d if resid[i] else None, hs[i], dprev, M, B, K, B, B, act,
                     LRELU_SLOPE)
                d = dprev
        return (None, None, None, *grads)


# ---------------------------------------------------------------------------------------------
# attention head
# ---------------------------------------------------------------------------------------------
class HeadTables:
    """Device-resident constants of the attention head for one (R, Ho, spacing, prior) configuration."""

    def __init__(self, R, Ho, spacing, rot_refinement, theta_prior, normal_prior_over_r, device):
        self.R, self.Ho, self.P = R, Ho, Ho * Ho
        p_r = tables.rotation_log_prior(R, rot_refinement, theta_prior, normal_prior_over_r)
        off = tables.rotation_offsets(R, rot_refinement)
        grid = tables.translation_grid(Ho, spacing)
        p_tr = tables.joint_log_prior(Ho, spacing, p_r)
        self.p_r = torch.from_numpy(p_r).to(device)
        self.off = torch.from_numpy(off).to(device)
        self.grid = torch.from_numpy(grid.astype(np.float32)).contiguous().to(device)
        self.p_tr = torch.from_numpy(p_tr).to(device)
        self.sigma_p = math.pi / R                       # train_mnist.py:269-272
        self.theta_off_scale = 1.0 if rot_refinement else 0.0


HEAD_REG_MAX = 9 * 1024


def head_reg_route(RP: int) -> bool:
    """Whether tvae_attn_head_fwd / _bwd run their register-resident kernels (csrc/abi_small.hip: head_reg_npt, the rule
    this restates for PATH_LOG): at most 9 positions for each of the 1024 threads of an image, TVAE_HEAD_REG=0 restores the
    strided kernels.  Read at every call, as the library does."""
    return 1 <= RP <= HEAD_REG_MAX and not os.environ.get('TVAE_HEAD_REG', '1').startswith('0')


class HeadFn(torch.autograd.Function):
    """Prior add + log-softmax + Gumbel-softmax (src/models.py:382-388) fused with expected-value pooling,
    reparameterised sampling, translation expectation and the KL block (train_mnist.py:192-231,242-282).

    Returns (attn, q_t_r, a_sampled) [B][R*P], z [B][zd], theta [B], dx [B][2], kl [B]."""

    @staticmethod
    def forward(ctx, heads, E, eps_z, eps_t, tb: HeadTables, B, zd):
        RP = tb.R * tb.P
        dev = heads.device
        _expect(tuple(heads.shape) == (3 + 2 * zd, B * RP), f'heads {tuple(heads.shape)} != ({3 + 2 * zd}, {B * RP})')
        _expect(E.numel() == B * RP and eps_z.numel() == B * zd and eps_t.numel() == B, 'noise shapes do not match')
        attn = torch.empty(B, RP, dtype=torch.float32, device=dev)
        q = torch.empty_like(attn)
        a = torch.empty_like(attn)
        z = torch.empty(B, zd, dtype=torch.float32, device=dev)
        th = torch.empty(B, dtype=torch.float32, device=dev)
        dx = torch.empty(B, 2, dtype=torch.float32, device=dev)
        kl = torch.empty(B, dtype=torch.float32, device=dev)
        heads = heads.contiguous()
        E, eps_z, eps_t = E.contiguous(), eps_z.contiguous(), eps_t.contiguous()
        part = _scratch(dev, 'head_part', 1024 * (7 + 3 * (zd + 1)))     # chunk partials (few images, many positions)
        if head_reg_route(RP):
            _note('head.reg')
        call('tvae_attn_head_fwd', heads, heads.shape[1], E, eps_z, eps_t, tb.p_r, tb.off, tb.p_tr, tb.grid, B, tb.R,
             tb.P, zd, tb.sigma_p, tb.theta_off_scale, attn, q, a, z, th, dx, kl, part, part.numel())
        ctx.save_for_backward(heads, q, a, eps_z, eps_t)
        ctx.tb, ctx.B, ctx.zd = tb, B, zd
        # outputs nothing differentiates (attn, q_t_r, a_sampled in the training step) reach backward as None, not as three
        # zero-filled [B][R P] tensors
        ctx.set_materialize_grads(False)
        return attn, q, a, z, th, dx, kl

    @staticmethod
    def backward(ctx, g_attn, g_q, g_a, g_z, g_th, g_dx, g_kl):
        heads, q, a, eps_z, eps_t = ctx.saved_tensors
        tb, B, zd = ctx.tb, ctx.B, ctx.zd
        dev = heads.device

        def dense(g, shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev) if g is None else g.contiguous()

        g_z, g_th, g_dx, g_kl = dense(g_z, (B, zd)), dense(g_th, (B,)), dense(g_dx, (B, 2)), dense(g_kl, (B,))
        opt = [None if g is None else g.contiguous() for g in (g_attn, g_q, g_a)]
        dheads = torch.empty_like(heads)
        part = _scratch(dev, 'head_part', 1024 * (7 + 3 * (zd + 1)))
        call('tvae_attn_head_bwd', heads, heads.shape[1], q, a, eps_z, eps_t, tb.p_r, tb.off, tb.p_tr, tb.grid, B,
             tb.R, tb.P, zd, tb.sigma_p, tb.theta_off_scale, g_z, g_th, g_dx, g_kl, opt[0], opt[1], opt[2], dheads,
             part, part.numel())
        return dheads, None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------
# coordinate transform, decoder, likelihood
# ---------------------------------------------------------------------------------------------
class CoordFn(torch.autograd.Function):
    """x' = (x - dx) R(theta) (train_mnist.py:222,234-239).  xc [Np][2] -> [B][Np][2]."""

    @staticmethod
    def forward(ctx, xc, dx, theta):
        B, Np = theta.shape[0], xc.shape[0]
        _expect(tuple(xc.shape) == (Np, 2) and tuple(dx.shape) == (B, 2) and theta.dim() == 1, 'coordinate shapes')
        xc, dx, theta = xc.contiguous(), dx.contiguous(), theta.contiguous()
        xr = torch.empty(B, Np, 2, dtype=torch.float32, device=xc.device)
        call('tvae_coord_fwd', xc, dx, theta, xr, B, Np)
        ctx.save_for_backward(xc, dx, theta)
        return xr

    @staticmethod
    def backward(ctx, g):
        xc, dx, theta = ctx.saved_tensors
        B, Np = theta.shape[0], xc.shape[0]
        gdx = torch.empty(B, 2, dtype=torch.float32, device=xc.device)
        gth = torch.empty(B, dtype=torch.float32, device=xc.device)
        call('tvae_coord_bwd', xc, dx, theta, g.contiguous(), gdx, gth, B, Np)
        return None, gdx, gth


DEC_PAD = os.environ.get('TVAE_DEC_PAD', '1') != '0'
DEC_LD_PAD = int(os.environ.get('TVAE_DEC_LD_PAD', '64'))


class DecoderRoute(NamedTuple):
    """Every structural decision of DecoderFn, taken once by decoder_route() in the forward and kept on ctx: the backward
    routes by it, so the two passes cannot disagree about what was stored, and with which row stride."""
    ldn: int             # row stride (floats) of every stored [features][B*Np] tensor
    split: bool          # hidden layers on the split pipe (tvae_linear_*_x6)
    four_x6: bool        # Fourier first layer on the split pipe, latent rows z[img(n)] joining the reduction
    four_dgrad_x6: bool  # its data gradient on the split pipe (Ff rows wide)
    virt_act: bool       # coordinate layer recomputed by its consumers, never stored; its backward in the first dgrad
    fused_out: bool      # the single-output Linear applied by the last hidden layer's launch
    virt_grad: bool      # last hidden layer's gradient Wo[f] gy[n] act'(h) re-formed by its consumers, never stored
    sign_bits: bool      # ... and [h > 0] kept as bits for it (two-valued form)
    no_h: bool           # last hidden activation neither stored nor read; its row sums come from the data gradient
    h3: bool             # two-part arithmetic with bound words for the operands streamed from memory
    infer: bool          # inference-mode forward: nothing is kept for a backward


def decoder_route(B: int, Np: int, F_: int, n_hidden: int, n_out: int, act: int, resid: bool, Ff: int,
                  infer: bool) -> DecoderRoute:
    """The route of DecoderFn for B images of Np pixels, F_ hidden units, Ff Fourier features (0: none) in the current
    arithmetic.  Pure: no tensor, no launch."""
    Nt = B * Np
    split = _dense_x6_ok(F_, Nt)
    virt_grad = n_hidden >= 1 and n_out == 1 and not resid and split
    sign_bits = virt_grad and act == ACT_LRELU
    # Row stride: the decoders that STORE activations and gradients (Fourier first layer, two or more hidden layers) stream
    # them again as the panels of their weight gradients; with a power-of-two column count (galaxy: 8 x 128^2 = 2^17) the 512
    # rows of a panel sit 2^19 bytes apart, every one in the same sets of the L2, and the four workgroups that share a panel
    # each fetch it again (1.88 GB fetched for 0.54 GB, profiles/r06_wgrad_probe.txt).  DEC_LD_PAD floats of padding per row
    # take the rows off that spacing.
    ld_pad = DEC_LD_PAD and (Ff or n_hidden >= 2) and Nt % 16384 == 0 and split      # (rows >= 64 KB x k apart)
    return DecoderRoute(
        ldn=Nt + DEC_LD_PAD if ld_pad else Nt, split=split, four_x6=bool(Ff) and split,
        four_dgrad_x6=bool(Ff) and _dense_x6_ok(Ff, Nt),
        virt_act=not Ff and n_hidden >= 1 and not resid and F_ <= 512 and Np % 128 == 0 and split,
        fused_out=n_hidden >= 1 and n_out == 1 and F_ <= 512 and split, virt_grad=virt_grad, sign_bits=sign_bits,
        no_h=sign_bits and F_ <= 512, h3=parts() == 2 and split, infer=infer)


class DecoderLayer(NamedTuple):
    """The launches of one hidden layer of DecoderFn (split-pipe routes; the f32 launches take none of it).  A bound is
    named by where it comes from, '' = none: the operand is exact, recomputed, or the launch runs three-part."""
    # forward (tvae_linear_fwd_x6)
    parts: int
    x_bound: str         # bound of the streamed input: 'virt' (recomputed coordinate layer: none needed), 'rows' (the first
    #                      layer's analytic bound), 'meas' (the maximum the layer in front left)
    y_max: bool          # leaves max |output| for the layer behind
    fused_out: bool      # applies the single-output Linear too
    store_h: bool        # writes its activation
    store_bits: bool     # writes [h > 0] as bits
    # backward
    virt_grad: bool      # its pre-activation gradient is re-formed from the saved activation / bits, not stored
    two_val: bool        # ... in the two-valued LeakyReLU form
    from_bits: bool      # ... with no stored activation: row sums and dWo come out of the two GEMMs
    wgrad_parts: int
    wgrad_bound: str     # 'two_val' (input bound x max |gy|), 'plain' (gradient word and input bound)
    wgrad_x_rows: bool   # ... the input bound is one value per unit (the row-sum chain exists), not a single word
    dgrad_parts: int
    d_bound: str         # bound word of the stored gradient it streams: 'top' (analytic, behind the output layer), 'meas'
    dgrad_max: bool      # the data gradient leaves max |result| for the layer in front
    fuse_in: bool        # the data gradient feeds the recomputed coordinate layer's backward; its result is not stored


class DecoderPlan(NamedTuple):
    """Arithmetic and bounds of every DecoderFn launch, decided once by decoder_plan() and kept on ctx with the route."""
    layers: tuple        # of DecoderLayer, one per hidden layer
    first_parts: int     # Fourier first layer on the split pipe (under max(1, max |z|) in h3)
    four_bound: str      # bound word of the gradient the Fourier layer's backward streams: 'top', 'two_val' (analytic, behind
    #                      a two-valued data gradient), 'meas'
    four_wgrad_parts: int
    four_dgrad_parts: int
    chain: bool          # per-unit analytic bounds of the stored activations (row-sum chain from the first layer)
    h_words: bool        # words for the measured maxima of the hidden activations
    top_bound: bool      # analytic bound word of the stored top gradient
    d_words: bool        # words for the measured maxima of the stored gradients


def decoder_plan(rt: DecoderRoute, n_hidden: int, resid: bool, fourier: bool) -> DecoderPlan:
    """Per-launch decisions of DecoderFn on route `rt` (which holds what the activation decides: sign_bits) in the current
    arithmetic.  Pure: no tensor, no launch.  The only place where the arithmetic turns into a `parts` value or a bound for
    the decoder; h3 (two parts) runs
      forward: the layer behind a recomputed coordinate layer; behind a stored first layer under its analytic bound (round
        4; a residual first hidden layer stays three-part); every deeper layer under the maximum the layer in front
        measured (round 6: an analytic chain would lose ~5 bits of fp16's exponent per layer);
      backward: the two-valued implicit gradient (exact 0 / 1 operand), and every stored gradient under its bound word
        -- the top one analytic, every later one measured by the data gradient that stores it."""
    return _decoder_plan(rt, n_hidden, resid, bool(fourier), parts(), _p3())


@functools.lru_cache(maxsize=None)
def _decoder_plan(rt, n_hidden, resid, fourier, p, p3):
    h3 = rt.h3
    layers = []
    for li in range(n_hidden):
        first, last = li == 0, li == n_hidden - 1
        virt_in = first and rt.virt_act
        x_bound = 'virt' if virt_in else '' if not h3 else 'meas' if not first else '' if resid else 'rows'
        virt_grad, two_val = last and rt.virt_grad, last and rt.sign_bits
        wgrad_bound = '' if (not h3 or virt_in or (virt_grad and not two_val)) else 'two_val' if two_val else 'plain'
        layers.append(DecoderLayer(
            parts=2 if (h3 and x_bound) else p3, x_bound=x_bound, y_max=h3 and not last, fused_out=last and rt.fused_out,
            store_h=not (last and rt.no_h), store_bits=two_val and not rt.infer,
            virt_grad=virt_grad, two_val=two_val, from_bits=last and rt.no_h,
            wgrad_parts=2 if (h3 and (two_val or wgrad_bound)) else p3, wgrad_bound=wgrad_bound,
            wgrad_x_rows=bool(wgrad_bound) and not rt.virt_act,
            dgrad_parts=2 if (h3 and (two_val or not virt_grad)) else p3,
            d_bound='' if (not h3 or virt_grad) else 'top' if last else 'meas',
            dgrad_max=h3 and (n_hidden >= 2 or fourier) and not virt_in, fuse_in=virt_in))
    four_bound = '' if not (h3 and fourier) else 'top' if not layers else 'two_val' if layers[0].two_val else 'meas'
    return DecoderPlan(
        layers=tuple(layers), first_parts=p, four_bound=four_bound, four_wgrad_parts=2 if four_bound else p3,
        four_dgrad_parts=2 if four_bound else p3, chain=h3 and not rt.virt_act, h_words=h3 and n_hidden >= 2,
        top_bound=h3 and not rt.virt_grad, d_words=h3 and (n_hidden >= 2 or fourier))


def decoder_padded_pixels(Np: int, B: int, F_: int, n_hidden: int, n_out: int, resid: bool, fourier: bool, act: int) -> int:
    """Round 5: images whose pixel count is not a multiple of the 128-column GEMM tile (28 x 28 = 784, 50 x 50 = 2 500) cannot
    take the decoder's fast path -- first layer recomputed inside its consumers, lean epilogues, fused first-layer backward --
    because its tiles must lie inside one image.  Padding every image's pixel range to the next multiple of 128 (coordinates
    (0, 0), outputs sliced away, zero upstream gradient: every reduction of the backward is unaffected) costs <= 15 % more
    columns and removes the stored first layer, its separate backward pass and the generic epilogues.  Returns the padded
    pixel count, or 0 when the decoder should run as it is (src/models.py: SpatialGenerator.forward pads around DecoderFn, so
    autograd differentiates the padding)."""
    Np_p = (Np + 127) // 128 * 128
    if (not DEC_PAD or Np % 128 == 0 or n_out != 1 or act != ACT_LRELU or Np_p > 1.15 * Np or
            not decoder_route(B, Np_p, F_, n_hidden, n_out, act, resid, int(fourier), False).virt_act):
        return 0
    return Np_p


class _DecoderBounds:
    """The h3 bound words of one DecoderFn call (include/tvae_hip.h: x_amax, a_amax, y_amax), formed as the plan asks and
    handed to the launches by where the plan says they come from.  Forward: rows[l], the per-unit analytic bound of the
    stored activation hs[l] (the first layer's, then |act(W h + b [+ h])| <= |W| rows + |b| [+ rows] unit by unit), and
    meas, one word per hidden activation that the launch storing it fills with its maximum.  Kept on ctx; begin_backward()
    adds the words of the stored gradients (dmeas) and max |gy|, formed on first use."""

    def __init__(self, plan: DecoderPlan, n_hidden: int, dev):
        self.plan, self.rows, self.h_bound = plan, [None], None
        self.meas = torch.zeros(max(n_hidden, 1), dtype=torch.float32, device=dev) if plan.h_words else None

    def _first(self, rows):
        self.rows, self.h_bound = [rows], rows.amax().reshape(1)

    def first_fourier(self, Wfull, bc, z_rows):
        """Fourier first layer: the streamed operand is cos(.) <= 1 over the latent rows, so its bound max(1, max |z|) is
        known without looking at it (returned); the layer's output is bounded by the absolute row sums of the weights."""
        feat_amax = torch.clamp(_inf_norm(z_rows), min=1.0) if z_rows is not None else \
            torch.ones(1, dtype=torch.float32, device=Wfull.device)
        self._first(Wfull.detach().abs().sum(1) * feat_amax + bc.detach().abs())
        return feat_amax

    def first_coord(self, xr, Wc, bc, LB):
        """The stored coordinate layer: |act(pre)| <= |pre| <= this bound."""
        self._first(_inf_norm(xr) * Wc.detach().abs().sum(1) +
                    ((bc.detach()[None, :] + LB).abs().amax(0) if LB is not None else bc.detach().abs()))

    def next_layer(self, W, b, resid):
        r = self.rows[-1]
        self.rows.append(torch.addmv(b.detach().abs(), W.detach().abs(), r) + (r if resid else 0.0)
                         if self.plan.chain else None)

    def fwd_x(self, li, lp):
        return self.h_bound if lp.x_bound == 'rows' else self.meas[li - 1:li] if lp.x_bound == 'meas' else None

    def fwd_y(self, li, lp):
        return self.meas[li:li + 1] if lp.y_max else None

    def begin_backward(self, gy, Wo, n_hidden):
        """(per backward call: nothing of an earlier one is reused.)  The top gradient's word: |d[m][n]| <=
        max_m sum_o |Wo[o][m]| max |gy| (act' <= 1).  Measured words only where a stored gradient is streamed again -- a
        second hidden layer, or the Fourier first layer behind the first one; other configurations launch no fill."""
        self.gy, self.gy_max = gy, None
        self.top = (self.gy_amax() * Wo.detach().abs().sum(0).amax()).reshape(1) if self.plan.top_bound else None
        self.dmeas = torch.zeros(n_hidden + 1, dtype=torch.float32, device=gy.device) if self.plan.d_words else None

    def gy_amax(self):
        if self.gy_max is None:
            self.gy_max = _inf_norm(self.gy)         # (one reduction over the output gradient)
        return self.gy_max

    def h_in(self, li):
        """Bound of hidden layer li's stored input: the first layer's analytic per-unit bound, or a deeper layer's measured
        maximum, capped unit by unit by the row-sum chain where the forward formed it (a unit far below the others keeps
        its own scale)."""
        if li == 0:
            return self.rows[0]
        m = self.meas[li - 1:li]
        return torch.minimum(self.rows[li], m) if self.plan.chain else m

    def wgrad_x(self, li, lp):
        """x_amax of layer li's weight gradient; the two-valued form's operand is gy[n] X[k][n] (vg_gy is gy: n_out == 1)."""
        return self.h_in(li) * self.gy_amax() if lp.wgrad_bound == 'two_val' else self.h_in(li) if lp.wgrad_bound else None

    def d_word(self, src, li):
        """Bound word of the stored gradient in front of hidden layer li (li = n_hidden: the top one; 'meas': what layer li's
        data gradient left)."""
        return self.top if src == 'top' else self.dmeas[li:li + 1] if src == 'meas' else None

    def behind_two_val(self, W, wo):
        """The gradient a two-valued data gradient leaves is read again by the Fourier first layer's backward, under this
        analytic bound: |dX[k][n]| <= max |gy| * sum_m |wo[m] W[m][k]|."""
        return self.gy_amax() * (W.detach().abs() * wo.detach().abs()[:, None]).sum(0).amax().reshape(1)

    def dgrad_y(self, li, lp):
        return self.dmeas[li:li + 1] if lp.dgrad_max else None


def _decoder_params(params, n_hidden):
    """DecoderFn's parameter tuple -> Wc, bc, Wl, [(W_i, b_i)], Wo, bo, Wf, bf (None where the model has none)."""
    Wc, bc, Wl = params[:3]
    Wo, bo, Wf, bf = params[3 + 2 * n_hidden:7 + 2 * n_hidden]
    return Wc, bc, Wl, [(params[3 + 2 * i], params[4 + 2 * i]) for i in range(n_hidden)], Wo, bo, Wf, bf


def _decoder_va(xr, Wc, bc, LB, Nt, Np):
    """Keyword group of the launches that recompute the coordinate layer's output instead of reading it (virt_act)."""
    return dict(va_xr=xr.view(Nt, 2), va_wc=Wc.contiguous(), va_bc=bc, va_lb=LB, va_np=Np)


class DecoderFn(torch.autograd.Function):
    """SpatialGenerator.forward (src/models.py:95-123): [Fourier] -> coord_linear + latent_linear -> act ->
    (Linear | ResidLinear, act) x (L-1) -> Linear(hid, n_out).  x [B][Np][2], z [B][zd] -> (B, Np, n_out).

    params order: Wc, bc, Wl (or None), [W_i, b_i]*(L-1), Wo, bo, then Fourier buffers Wf, bf (or None)."""

    @staticmethod
    def forward(ctx, xr, z, act, resid, sigma, n_hidden, *params):
        Wc, bc, Wl, hidden, Wo, bo, Wf, bf = _decoder_params(params, n_hidden)
        xr = xr.contiguous()
        _expect(xr.dim() == 3 and xr.shape[2] == 2, f'decoder coordinates {tuple(xr.shape)} are not (B, N, 2)')
        B, Np = xr.shape[0], xr.shape[1]
        Nt = B * Np
        F_, n_out = Wc.shape[0], Wo.shape[0]
        _expect(1 <= n_out <= 4, f'n_out = {n_out} (the skinny output kernels handle 1..4)')
        _expect(Wc.shape[1] == (Wf.shape[0] if Wf is not None else 2) and Wo.shape[1] == F_ and
                all(tuple(W.shape) == (F_, F_) for W, _ in hidden), 'decoder parameter shapes are inconsistent')
        _expect(Wl is None or (z is not None and tuple(z.shape) == (B, Wl.shape[1])), 'latent z does not match latent_linear')
        dev = xr.device
        rt = decoder_route(B, Np, F_, n_hidden, n_out, act, resid, Wf.shape[0] if Wf is not None else 0, _INFER)
        plan = decoder_plan(rt, n_hidden, resid, Wf is not None)
        bd = _DecoderBounds(plan, n_hidden, dev)
        ldn = rt.ldn
        LB = None
        if ldn != Nt:
            _note('dec.ld_pad')
        # Fourier-feature first layer on the split pipe (four_x6): the per-image latent term joins the reduction (rows
        # z[img(n)] under the features, weights [Wc | Wl]) instead of being a per-image bias
        if Wl is not None:
            z = z.contiguous()
        if Wl is not None and not rt.four_x6:
            zd = Wl.shape[1]
            LB = torch.empty(B, F_, dtype=torch.float32, device=dev)
            call('tvae_latent_bias', Wl.contiguous(), z, LB, B, F_, zd)
        feat = None
        # without Fourier features the coordinate layer's output is two FMAs and an activation per element: the layers
        # that consume it (first hidden layer: forward, mask of the data gradient, weight gradient) recompute it and the
        # [hid][B*n^2] tensor is never written or read (virt_act)
        va = _decoder_va(xr, Wc, bc, LB, Nt, Np) if rt.virt_act else None
        h = None if rt.virt_act else torch.empty(F_, ldn, dtype=torch.float32, device=dev)
        if rt.virt_act:
            _note('dec.virt_act')
        elif Wf is not None:
            Ff = Wf.shape[0]
            zx = Wl.shape[1] if (rt.four_x6 and Wl is not None) else 0
            feat_all = torch.empty(Ff + zx, ldn, dtype=torch.float32, device=dev)
            feat = feat_all[:Ff]
            call('tvae_fourier_fwd', xr, Wf.contiguous(), bf.contiguous(), sigma, feat, ldn, Ff, Nt)
            if rt.four_x6:
                _note('dec.four_x6')
                if zx:
                    feat_all[Ff:, :Nt].view(zx, B, Np).copy_(z.contiguous().t().unsqueeze(2).expand(zx, B, Np))
                Wfull = torch.cat([Wc, Wl], 1) if zx else Wc
                feat_amax = None
                if plan.chain:                         # (h3, round 4)
                    feat_amax = bd.first_fourier(Wfull, bc, z if zx else None)
                    _note('dec.four_h3')
                w3c = _split_weight(Wfull, F_, Ff + zx, False, 'x6_dense_wc', nparts=plan.first_parts)
                with _timed('tvae_linear_fwd_x6', plan.first_parts):
                    call('tvae_linear_fwd_x6', w3c, feat_all, bc, None, h, F_, Nt, Ff + zx, ldn, ldn, act, LRELU_SLOPE,
                         parts=plan.first_parts, x_amax=feat_amax)
            else:
                call('tvae_linear_fwd', Wc.contiguous(), feat, bc, LB, Np, None, h, F_, Nt, Ff, ldn, ldn, act, LRELU_SLOPE)
        else:
            call('tvae_dec_l0_fwd', xr, Wc.contiguous(), bc, LB, h, ldn, F_, Nt, Np, act, LRELU_SLOPE)
            if plan.chain:
                bd.first_coord(xr, Wc, bc, LB)
        hs = [h]
        yh = torch.empty(B, Np, n_out, dtype=torch.float32, device=dev)
        sbits = None
        for li, ((W, b), lp) in enumerate(zip(hidden, plan.layers)):
            hn = None
            if rt.split:
                if lp.x_bound in ('rows', 'meas'):
                    _note('dec.hidden_h3_mem' if lp.x_bound == 'rows' else 'dec.hidden_h3_meas')
                w3 = _split_weight(W, F_, F_, False, 'x6_dense_w', nparts=lp.parts)
                # the backward of the single-output Linear behind the last hidden layer needs only the SIGN of this
                # layer's LeakyReLU output (two-valued implicit gradient): one bit per element, stored by this launch
                if lp.store_bits:
                    sbits = torch.empty(F_, Nt // 32, dtype=torch.int32, device=dev)
                    _note('dec.sign_bits')
                # Round 4: with the fused output dot AND the sign bits, nothing downstream needs this layer's activation
                # itself -- the backward takes [H > 0] from the bits and dWo from the identity sum_k W[m][k] G[m][k] +
                # b[m] g0[m] (include/tvae_hip.h: tvae_linear_dgrad_x6 vg_bits) -- so the 2.1 GB tensor is neither written
                # here nor read there.  (inference: same launch without the bits -- only the fused output dot leaves it)
                if lp.store_h:
                    hn = torch.empty(F_, ldn, dtype=torch.float32, device=dev)
                else:
                    _note('dec.no_h_inference' if rt.infer else 'dec.no_h')
                # the last hidden layer also applies the single-output Linear that follows it (one pass less over h)
                with _timed('tvae_linear_fwd_x6', lp.parts):
                    call('tvae_linear_fwd_x6', w3, hs[-1], b, hs[-1] if resid else None, hn, F_, Nt, F_, ldn, ldn, act,
                         LRELU_SLOPE, **(dict(col_w=Wo.contiguous(), col_b=bo, col_y=yh) if lp.fused_out else {}),
                         **(va if lp.x_bound == 'virt' else {}), sign_bits=sbits, parts=lp.parts, x_amax=bd.fwd_x(li, lp),
                         y_amax=bd.fwd_y(li, lp))
                _note('dec.fused_out' if lp.fused_out else 'dec.hidden_x6')
            else:
                hn = torch.empty(F_, ldn, dtype=torch.float32, device=dev)
                call('tvae_linear_fwd', W.contiguous(), hs[-1], b, None, 1, hs[-1] if resid else None, hn, F_, Nt, F_,
                     ldn, ldn, act, LRELU_SLOPE)
            bd.next_layer(W, b, resid)
            hs.append(hn)
        if not rt.fused_out:
            call('tvae_coldot', hs[-1], ldn, F_, Nt, Wo.contiguous(), 1, F_, bo, n_out, yh)
        if rt.infer:
            return yh
        ctx.save_for_backward(xr, z if Wl is not None else None, feat, LB if rt.virt_act else None, *hs, *params)
        ctx.meta = (act, resid, sigma, n_hidden, B, Np)
        ctx.arith = get_gemm_mode()
        ctx.route, ctx.plan, ctx.bounds, ctx.sbits = rt, plan, bd, sbits
        return yh

    @staticmethod
    @_in_forward_arithmetic
    def backward(ctx, gy):
        act, resid, sigma, n_hidden, B, Np = ctx.meta
        rt, plan, bd = ctx.route, ctx.plan, ctx.bounds
        sv = ctx.saved_tensors
        xr, z, feat, LB = sv[:4]
        hs = sv[4:5 + n_hidden]
        Wc, bc, Wl, hidden, Wo, bo, Wf, bf = _decoder_params(sv[5 + n_hidden:], n_hidden)
        Nt = B * Np
        F_, n_out = Wc.shape[0], Wo.shape[0]
        dev = xr.device
        ldn = rt.ldn                                     # (row stride of every stored [features][Nt] tensor)
        gy = gy.contiguous().view(Nt, n_out)
        bd.begin_backward(gy, Wo, n_hidden)
        # last layer: one pass over h gives d (pre-activation gradient), its row sums and dWo
        gyT = gy.t().contiguous()
        dbo = _rowsum(gyT, n_out, Nt)
        # with a single output the gradient of the last hidden activation, Wo[f] gy[n] act'(h[f][n]), is cheap to
        # re-form inside the two GEMMs that consume it: it is then never written (dec_out_bwd only produces row sums)
        d = None if rt.virt_grad else torch.empty(F_, ldn, dtype=torch.float32, device=dev)
        tot = torch.empty(1 + n_out, F_, dtype=torch.float32, device=dev)      # tot[0]: bias gradient of the last hidden layer
        # two-valued implicit gradient without the saved activation: the data-gradient launch of the last hidden layer
        # streams the sign bits anyway and returns the two row sums this layer's backward needs (tot[0], tot[1] = dWo): no
        # pass of its own
        if not rt.no_h:
            part = workspace(dev, ((Nt + 1023) // 1024) * F_ * (1 + n_out))
            call('tvae_dec_out_bwd', gy, n_out, Wo.contiguous(), hs[-1], ldn, d, ldn, F_, Nt, act, LRELU_SLOPE, part,
                 part.numel(), tot)
        else:
            _note('dec.row_sums_in_dgrad')
        vg = dict(vg_wo=Wo.contiguous().view(-1), vg_gy=gy.view(-1), vg_act=act) if rt.virt_grad else None
        if rt.virt_grad:
            _note('dec.virt_grad')
        va = _decoder_va(xr, Wc, bc, LB, Nt, Np) if rt.virt_act else None
        dWo = tot[1:]
        grads_hidden = []
        for li in range(n_hidden - 1, -1, -1):
            (W, b), lp, hprev = hidden[li], plan.layers[li], hs[li]
            dsrc = hs[-1] if lp.virt_grad else d       # implicit operand: pass the saved activation instead
            sbits = ctx.sbits if lp.two_val else None  # [h > 0] as stored bits
            d_bnd = bd.d_word(lp.d_bound, li + 1)
            if lp.wgrad_bound == 'plain':
                _note('dec.wgrad_h3_meas')
            # from_bits: the weight gradient also returns rowdot[m] = sum_k W[m][k] G[m][k] for dWo, and the data gradient
            # below the two row sums of the layer behind
            wg = _wgrad(dsrc, hprev, F_, Nt, F_, vg if lp.virt_grad else None, va if lp.x_bound == 'virt' else None, act,
                        sbits, rowdot_w=W if lp.from_bits else None, a_amax=d_bnd if lp.wgrad_bound == 'plain' else None,
                        x_amax=bd.wgrad_x(li, lp), ld=ldn, nparts=lp.wgrad_parts, x_amax_rows=lp.wgrad_x_rows,
                        two_val=lp.two_val)
            dW, rowdot = wg if lp.from_bits else (wg, None)
            db = tot[0] if li == n_hidden - 1 else _rowsum(d, F_, Nt, ld=ldn)
            # the data gradient of the FIRST hidden layer behind a recomputed coordinate layer feeds that layer's backward
            # from its epilogue (coordinate gradient + per-panel row sums); its result is then never written
            dprev = None if lp.fuse_in else torch.empty(F_, ldn, dtype=torch.float32, device=dev)
            if rt.split:
                p_d = lp.dgrad_parts
                if lp.d_bound:
                    _note('dec.dgrad_h3_meas')
                if lp.two_val:                         # LeakyReLU: 3 MFMAs per block instead of 6
                    w3t, csum = _split_weight(W, F_, F_, True, 'x6_dense_wt', scale=vg['vg_wo'], nparts=p_d)
                    _note('dec.virt_grad_2val')
                else:
                    w3t, csum = _split_weight(W, F_, F_, True, 'x6_dense_wt', nparts=p_d), None
                fin = {}
                if lp.fuse_in:
                    gxr_f = torch.empty(B, Np, 2, dtype=torch.float32, device=dev)
                    part_f = workspace(dev, (Nt // 128) * F_ * 3)
                    fin = dict(in_xr=xr.view(Nt, 2), in_wc=Wc.contiguous(), in_gxr=gxr_f, in_part=part_f,
                               in_part_floats=part_f.numel(), in_bc=bc, in_lb=LB, in_np=Np)
                rs_part = _scratch(dev, 'dec_rs_part', (Nt // 128) * F_ * 2) if lp.from_bits else None
                rs = dict(rs_part=rs_part, rs_part_floats=rs_part.numel(), rs_wo=vg['vg_wo'], rs_gysum=dbo, rs_db=tot[0],
                          rs_dwo=tot[1], vg_bits=sbits, rs_rowdot=rowdot, rs_bias=b) if lp.from_bits else {}
                with _timed('tvae_linear_dgrad_x6', p_d, lp.two_val):
                    call('tvae_linear_dgrad_x6', w3t, dsrc, d if resid else None, hprev, dprev, F_, Nt, F_, ldn, ldn, act,
                         LRELU_SLOPE, **fin, vg_wo=vg['vg_wo'] if (lp.virt_grad and not lp.two_val) else None,
                         vg_gy=vg['vg_gy'] if lp.virt_grad else None, vg_csum=csum, **rs, parts=p_d, x_amax=d_bnd,
                         y_amax=bd.dgrad_y(li, lp))
                if lp.fuse_in:
                    _note('dec.fuse_in')
            else:
                call('tvae_linear_dgrad', W.contiguous(), d, d if resid else None, hprev, dprev, F_, Nt, F_, ldn, ldn,
                     act, LRELU_SLOPE)
            d = dprev
            grads_hidden.append((dW, db))
        grads_hidden.reverse()
        # first layer: d is the pre-activation gradient [F][Nt]
        Simg = torch.empty(B, F_, dtype=torch.float32, device=dev)
        dbc = torch.empty(F_, dtype=torch.float32, device=dev)
        gxr = gxr_f if rt.virt_act else torch.empty(B, Np, 2, dtype=torch.float32, device=dev)
        if rt.virt_act:
            dWc = torch.empty(F_, 2, dtype=torch.float32, device=dev)
            call('tvae_dec_in_total', part_f, B, Np // 128, F_, Simg, dbc, dWc)
        elif Wf is not None:
            call('tvae_rowdot_seg', d, ldn, None, 1, F_, Nt, Np, Simg)
            call('tvae_seg_sum', Simg, B, F_, dbc, 1.0, 0)
        else:
            # one pass over d: coordinate gradient, per-image sums, bias and coordinate-weight gradients
            dWc = torch.empty(F_, 2, dtype=torch.float32, device=dev)
            part = workspace(dev, B * ((Np + 1023) // 1024) * F_ * 3)
            call('tvae_dec_in_bwd', d, ldn, xr.view(Nt, 2), Wc.contiguous(), F_, B, Np, gxr, Simg, dbc, dWc, part,
                 part.numel())
        dWl = dz = None
        if Wl is not None:
            zd = Wl.shape[1]
            dWl = torch.empty(F_, zd, dtype=torch.float32, device=dev)
            dz = torch.empty(B, zd, dtype=torch.float32, device=dev)
            call('tvae_latent_bwd', Simg, Wl.contiguous(), z, dWl, dz, B, F_, zd)
        if Wf is not None:
            Ff = Wf.shape[0]
            # h3 for the Fourier first layer's backward (round 4): both operands come from memory with known bounds -- the
            # features are cosines (<= 1), d is under its bound word (analytic behind a two-valued data gradient, else measured)
            d_bnd = bd.behind_two_val(hidden[0][0], vg['vg_wo']) if plan.four_bound == 'two_val' else \
                bd.d_word(plan.four_bound, 0)
            one = torch.ones(1, dtype=torch.float32, device=dev) if plan.four_bound else None
            dWc = _wgrad(d, feat, F_, Nt, Ff, a_amax=d_bnd, x_amax=one, ld=ldn, nparts=plan.four_wgrad_parts)
            dfeat = torch.empty(Ff, ldn, dtype=torch.float32, device=dev)
            if rt.four_dgrad_x6:
                p_f = plan.four_dgrad_parts
                w3t = _split_weight(Wc, Ff, F_, True, 'x6_dense_wct', nparts=p_f)
                with _timed('tvae_linear_dgrad_x6', p_f):
                    call('tvae_linear_dgrad_x6', w3t, d, None, None, dfeat, F_, Nt, Ff, ldn, ldn, ACT_NONE, LRELU_SLOPE,
                         parts=p_f, x_amax=d_bnd)
            else:
                call('tvae_linear_dgrad', Wc.contiguous(), d, None, None, dfeat, F_, Nt, Ff, ldn, ldn, ACT_NONE, LRELU_SLOPE)
            call('tvae_fourier_bwd', xr, Wf.contiguous(), bf.contiguous(), sigma, dfeat, ldn, Ff, Nt, gxr)
        out = [gxr, dz, None, None, None, None, dWc, dbc, dWl]
        for (dW, db) in grads_hidden:
            out += [dW, db]
        out += [dWo, dbo, None, None]
        return tuple(out)


LIK_KIND = {'bce': 0, 'bce3': 0, 'gauss': 1, 'gauss_var': 2}


class LogLikFn(torch.autograd.Function):
    """Per-image log-likelihood over flat vectors (train_mnist.py:288-291; train_galaxy.py:288-292;
    train_particles.py:284-296,336-338).  yh (B, ...), y (B, ...) -> lp [B]."""

    @staticmethod
    def forward(ctx, yh, y, kind):
        B = y.shape[0]
        ctx.shape = tuple(yh.shape)
        y = y.contiguous().view(B, -1)
        yh = yh.contiguous().view(B, -1)
        L = y.shape[1]
        assert yh.shape[1] == (2 * L if kind == 2 else L), (yh.shape, y.shape, kind)
        lp = torch.empty(B, dtype=torch.float32, device=yh.device)
        call('tvae_loglik_fwd', yh, y, lp, B, L, kind)
        ctx.save_for_backward(yh, y)
        ctx.kind = kind
        return lp

    @staticmethod
    def backward(ctx, g):
        yh, y = ctx.saved_tensors
        B, L = y.shape
        gyh = torch.empty_like(yh)
        call('tvae_loglik_bwd', yh, y, g.contiguous(), gyh, B, L, ctx.kind)
        return gyh.view(ctx.shape), None, None


class ElboFn(torch.autograd.Function):
    """(elbo f64, log_p f32, kl f64) of a minibatch from the per-image terms lp [B], kl [B] (train_mnist.py:282,291-292:
    log_p = lp.mean(), kl_div = kl.double().mean(), elbo = log_p - kl_div) -- one launch forward, one backward, instead of a
    dozen ATen launches for two means, a cast, a subtraction and their chain rules."""

    @staticmethod
    def forward(ctx, lp, kl):
        B = lp.shape[0]
        _expect(lp.dim() == 1 and tuple(kl.shape) == (B,) and B >= 1, 'per-image ELBO terms must be [B] vectors')
        dev_ = lp.device
        elbo = torch.empty((), dtype=torch.float64, device=dev_)
        logp = torch.empty((), dtype=torch.float32, device=dev_)
        kld = torch.empty((), dtype=torch.float64, device=dev_)
        call('tvae_elbo_reduce', lp.contiguous(), kl.contiguous(), B, elbo, logp, kld)
        ctx.B = B
        ctx.set_materialize_grads(False)
        return elbo, logp, kld

    @staticmethod
    def backward(ctx, g_elbo, g_logp, g_kld):
        B = ctx.B
        ref = next(g for g in (g_elbo, g_logp, g_kld) if g is not None)
        g_lp = torch.empty(B, dtype=torch.float32, device=ref.device)
        g_kl = torch.empty(B, dtype=torch.float32, device=ref.device)

        def as_(g, dt):
            return None if g is None else g.to(dt).contiguous()

        call('tvae_elbo_reduce_bwd', as_(g_elbo, torch.float64), as_(g_logp, torch.float32), as_(g_kld, torch.float64), B, g_lp,
             g_kl)
        return g_lp, g_kl


class CtfFn(torch.autograd.Function):
    """Per-image CTF filter of the reconstruction (train_particles.py:298-302): depthwise cross-correlation with an
    odd kernel, zero padding kc//2.  y_mu (B, n*n), ctf (B, 1, kc, kc) -> (B, n*n).  The filters are constants."""

    @staticmethod
    def forward(ctx, y_mu, ctf, n):
        B, kc = ctf.shape[0], ctf.shape[-1]
        _expect(kc % 2 == 1 and ctf.numel() == B * kc * kc and y_mu.numel() == B * n * n,
                f'CTF filters {tuple(ctf.shape)} / reconstruction {tuple(y_mu.shape)} do not match n = {n}')
        y_mu = y_mu.contiguous()
        ctf = ctf.contiguous()
        out = torch.empty_like(y_mu)
        call('tvae_ctf_corr', y_mu, ctf, out, B, n, kc, 0)
        ctx.save_for_backward(ctf)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, g):
        (ctf,) = ctx.saved_tensors
        B, kc = ctf.shape[0], ctf.shape[-1]
        gi = torch.empty_like(g)
        call('tvae_ctf_corr', g.contiguous(), ctf, gi, B, ctx.n, kc, 1)
        return gi, None, None


class MaskedLogLikFn(torch.autograd.Function):
    """Gaussian log-likelihood inside a circle of `radius` pixels centred at the inferred translation
    (train_particles.py:309-333,338).  The mask is built on the device from dx (the reference builds it on the host
    with numpy every step); it carries no gradient, like the reference's dx.detach()."""

    @staticmethod
    def forward(ctx, yh, y, dx, spacing, radius, n):
        B = y.shape[0]
        ctx.shape = tuple(yh.shape)
        _expect(yh.numel() == B * n * n and y.numel() == B * n * n and tuple(dx.shape) == (B, 2), 'masked likelihood shapes')
        yh = yh.contiguous().view(B, -1)
        y = y.contiguous().view(B, -1)
        dx = dx.detach().contiguous()
        lp = torch.empty(B, dtype=torch.float32, device=yh.device)
        call('tvae_loglik_masked_fwd', yh, y, dx, 1.0 / spacing, float(radius), B, n, lp)
        ctx.save_for_backward(yh, y, dx)
        ctx.cfg = (spacing, radius, n)
        return lp

    @staticmethod
    def backward(ctx, g):
        yh, y, dx = ctx.saved_tensors
        spacing, radius, n = ctx.cfg
        gyh = torch.empty_like(yh)
        call('tvae_loglik_masked_bwd', yh, y, dx, 1.0 / spacing, float(radius), y.shape[0], n, g.contiguous(), gyh)
        return gyh.view(ctx.shape), None, None, None, None, None


def adam_flat(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """Fused Adam on flat buffers (torch.optim.Adam defaults; reference train_mnist.py:579,323)."""
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    call('tvae_adam_flat', p, g, m, v, p.numel(), lr, b1, b2, eps, bc1, math.sqrt(bc2), grad_scale)
