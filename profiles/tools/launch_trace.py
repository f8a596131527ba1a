"""Host-side launch trace of the encoder-side Functions (EncoderFn, TransAttnEncoderFn, GroupConvFn) and of DecoderFn:
which entry points a configuration launches, in which order, with which scalars and which buffers.  No GPU and no built
library: `ops.call` is replaced by a recorder and `ops.query` by a fixed stub, the Functions run forward and backward on
CPU tensors.  The encoder side never looks at their contents; the decoder forms its h3 bound words from them with torch
operations, so its trace also takes those words by value and counts the ATen operations of a configuration.  Prints one
SHA-256 per sweep (encoder side, decoder), to compare two trees:

    python profiles/tools/launch_trace.py [TREE]        # TREE: the checkout whose tvae package is traced (default: this one)
"""
import contextlib
import functools
import hashlib
import itertools
import os
import sys
import types

import torch
from torch.utils._python_dispatch import TorchDispatchMode

SIZE = 4096              # what every size query answers (bytes or floats)
B, R, K, PAD = 2, 4, 3, 1
MODES = ('f32', 'x6', 'h3', 'bf16')
HEAD_ROWS = (3, 7, 8, 23, 103, 128, 129)
IMAGE = (8, 7)           # Ho = n: N = B R n^2 = 512 (a multiple of 32) and 392 (not one)
CONV = {'dft': ('tvae_conv1_dft_supported', 'tvae_conv1_x6_supported'), 'x6': ('tvae_conv1_x6_supported',), 'none': ()}


@contextlib.contextmanager
def traced(supported=()):
    """Inside: every ops.call is recorded instead of launched -- (name, arguments), a tensor as (shape, dtype, number of its
    buffer in order of first use) -- and ops.query answers `name in supported` to *_supported, 0 to *_ring, SIZE to the
    rest.  Yields the record: .launches, .paths (PATH_LOG), .parts (PARTS_LOG), and .bounds: (launch, argument, values) of
    every tensor passed as x_amax / a_amax.  A tensor passed as y_amax is filled with +inf, as if the kernel had left a
    maximum there: a bound that takes min(row-sum chain, measured word) then shows its chain; the per-image latent bias is
    computed, since a bound is formed from it.  .quiet is set while the
    recorder itself works (AtenCount skips what it does)."""
    from tvae import _lib, ops
    rec = types.SimpleNamespace(launches=[], paths=set(), parts={}, bounds=[], quiet=False)
    ids, alive = {}, []          # (every buffer is kept alive, so no address is handed out twice within a run)

    def arg(a):
        if not torch.is_tensor(a):
            return a
        alive.append(a)
        return tuple(a.shape), str(a.dtype), ids.setdefault((a.untyped_storage().data_ptr(), a.storage_offset()), len(ids))

    def call(name, *args, **kwargs):
        rec.quiet = True
        if kwargs:                   # the complete tuple: what the same launch written without keywords records
            args = _lib.bind_args(name, args, kwargs)
        if name in _lib.ARG_NAMES:
            words = _lib.ARG_NAMES[name].replace('|', ' ').replace('!', '').split()
            for w, a in zip(words, _lib.bind_args(name, args, {})):
                if torch.is_tensor(a) and w in ('x_amax', 'a_amax'):
                    rec.bounds.append((len(rec.launches), w, repr(a.tolist())))
                elif torch.is_tensor(a) and w == 'y_amax':
                    a.fill_(float('inf'))
        if name == 'tvae_latent_bias':       # (Wl, z, LB, ...): the one kernel output a bound is formed from (the stored
            args[2].copy_(args[1] @ args[0].t())         # coordinate layer's, DecoderFn), so the recorder computes it
        rec.launches.append((name,) + tuple(arg(a) for a in args))
        rec.quiet = False

    def query(name, *args):
        return int(name in supported) if name.endswith('_supported') else 0 if name.endswith('_ring') else SIZE

    saved = ops.call, ops.query, ops.PATH_LOG, ops.PARTS_LOG
    ops.call, ops.query, ops.PATH_LOG, ops.PARTS_LOG = call, query, rec.paths, rec.parts
    try:
        yield rec
    finally:
        ops.call, ops.query, ops.PATH_LOG, ops.PARTS_LOG = saved


def operands(which, C, nh, n, bias=True):
    """The Function and its arguments: 'encoder', 'trans_attn', 'trans_attn_plain' (--groupconv 0), 'groupconv'."""
    from tvae import ops

    def p(*shape):
        return torch.zeros(*shape, requires_grad=True)
    y = torch.zeros(B, 1, n, n)
    tail = (p(C, C), p(C), p(nh, C), p(nh))
    if which == 'encoder':
        return ops.EncoderFn, (y, p(C, 1, 1, K, K), p(C)) + tail
    if which == 'trans_attn':
        return ops.TransAttnEncoderFn, (y, p(C, 1, 1, K, K), p(C), p(1, R), p(1)) + tail
    if which == 'trans_attn_plain':
        return ops.TransAttnEncoderFn, (y, p(C, 1, K, K), p(C), None, None) + tail
    return ops.GroupConvFn, (y, p(C, 1, 1, K, K), p(C) if bias else None)


def trace(which, mode, nh, act, n, conv='dft', C=128, infer=False, bias=True):
    """Forward (+ backward unless `infer`) of one configuration under the stubs; returns the record of traced()."""
    from tvae import ops
    from tvae._lib import arithmetic
    fn, args = operands(which, C, nh, n, bias)
    args += (R, PAD) if which == 'groupconv' else (R, PAD, act)
    with arithmetic(mode), ops.inference(infer), traced(CONV[conv]) as rec:
        if infer:
            with torch.no_grad():
                fn.apply(*args)
        else:
            fn.apply(*args).sum().backward()
    return rec


def names(rec):
    return [l[0] for l in rec.launches]


# ATen operations that only make a view or an uninitialised buffer: not part of the decoder's bound arithmetic
METADATA_OPS = ('view', 'slice', 'select', 't', 'transpose', 'expand', 'unsqueeze', 'detach', 'alias', 'split')
METADATA_PREFIXES = ('empty', 'new_empty')


class AtenCount(TorchDispatchMode):
    """Counts the ATen operations that run inside (METADATA_OPS and the recorder's own work left out) into rec.aten."""

    def __init__(self, rec):
        super().__init__()
        self.rec = rec
        rec.aten = {}

    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        op = func.overloadpacket.__name__
        if not (self.rec.quiet or op in METADATA_OPS or op.startswith(METADATA_PREFIXES)):
            self.rec.aten[op] = self.rec.aten.get(op, 0) + 1
        return func(*args, **(kwargs or {}))


DEC_SIGMA = 0.5          # Fourier length scale handed to DecoderFn (a scalar of tvae_fourier_fwd / _bwd)


@functools.lru_cache(maxsize=32)
def decoder_data(B, Np, F_, n_hidden, n_out, Ff, zd):
    """Seeded random values of DecoderFn's operands: xr, z, params in its order (None where absent), output weights."""
    torch.manual_seed(1000 * n_hidden + 10 * zd + n_out)
    r = torch.randn
    params = [r(F_, Ff or 2), r(F_), r(F_, zd) if zd else None]
    for _ in range(n_hidden):
        params += [r(F_, F_), r(F_)]
    params += [r(n_out, F_), r(n_out), r(Ff, 2) if Ff else None, r(Ff) if Ff else None]
    return r(B, Np, 2), r(B, zd) if zd else None, params, r(B, Np, n_out)


def trace_decoder(mode, B, Np, F_, n_hidden, n_out, act, resid, Ff, zd, infer=False):
    """DecoderFn forward (+ backward unless `infer`) of one configuration under the stubs, on seeded random operands (the
    analytic bounds are formed from them); returns the record of traced(), with .aten: ATen operation -> count."""
    from tvae import ops
    from tvae._lib import arithmetic

    def leaf(t):
        return None if t is None else t.detach().requires_grad_()
    xr, z, params, weight = decoder_data(B, Np, F_, n_hidden, n_out, Ff, zd)     # (weight: the upstream gradient)
    xr, z, params = leaf(xr), leaf(z), [leaf(t) for t in params[:-2]] + params[-2:]
    with arithmetic(mode), ops.inference(infer), traced() as rec, AtenCount(rec):
        if infer:
            with torch.no_grad():
                ops.DecoderFn.apply(xr, z, act, resid, DEC_SIGMA, n_hidden, *params)
        else:
            (ops.DecoderFn.apply(xr, z, act, resid, DEC_SIGMA, n_hidden, *params) * weight).sum().backward()
    return rec


DEC_IMAGES = ((2, 128), (2, 100), (1, 16384))    # (B, Np): tile-aligned, not aligned (plain first layer), padded row stride
DEC_HIDDEN = (128, 256, 512, 1024)               # F_: below the split pipe, both sides of every F_ <= 512 test


def sweep_decoder():
    from tvae import ops
    h, count = hashlib.sha256(), 0
    for cfg in itertools.product(MODES, DEC_IMAGES, DEC_HIDDEN, (0, 1, 2, 3), (1, 3), (ops.ACT_LRELU, ops.ACT_TANH),
                                 (False, True), (0, 256), (0, 3), (False, True)):
        mode, (B_, Np), *rest = cfg
        rec = trace_decoder(mode, B_, Np, *rest)
        h.update(repr((cfg, rec.launches, rec.bounds, sorted(rec.paths), sorted(rec.parts.items()),
                       sorted(rec.aten.items()))).encode())
        count += 1
    return h.hexdigest(), count


def sweep():
    from tvae import ops
    h, count = hashlib.sha256(), 0
    for cfg in itertools.product(MODES, HEAD_ROWS, (ops.ACT_LRELU, ops.ACT_TANH), IMAGE, sorted(CONV), (128, 64),
                                 (False, True)):
        for which, bias in (('encoder', True), ('trans_attn', True), ('trans_attn_plain', True), ('groupconv', True),
                            ('groupconv', False)):
            rec = trace(which, *cfg, bias=bias)
            h.update(repr((which, bias, cfg, rec.launches, sorted(rec.paths), sorted(rec.parts.items()))).encode())
        count += 1
    return h.hexdigest(), count


if __name__ == '__main__':
    tree = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.join(tree, 'target-vae_amd'))
    torch.set_num_threads(1)     # (thousands of small reductions: a thread pool only adds its start-up to each)
    for side, run in (('encoder side', sweep), ('decoder', sweep_decoder)):
        digest, count = run()
        print('%s  %d configurations  %s  %s' % (digest, count, side, os.path.abspath(tree)))
