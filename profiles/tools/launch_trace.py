"""Host-side launch trace of the encoder-side Functions (EncoderFn, TransAttnEncoderFn, GroupConvFn): which entry points
a configuration launches, in which order, with which scalars and which buffers.  No GPU and no built library: `ops.call`
is replaced by a recorder and `ops.query` by a fixed stub, the Functions run forward and backward on CPU tensors (whose
contents are never looked at).  Prints one SHA-256 over the whole sweep, to compare two trees:

    python profiles/tools/launch_trace.py [TREE]        # TREE: the checkout whose tvae package is traced (default: this one)
"""
import contextlib
import hashlib
import itertools
import os
import sys
import types

import torch

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
    rest.  Yields the record: .launches, .paths (PATH_LOG), .parts (PARTS_LOG)."""
    from tvae import _lib, ops
    rec = types.SimpleNamespace(launches=[], paths=set(), parts={})
    ids, alive = {}, []          # (every buffer is kept alive, so no address is handed out twice within a run)

    def arg(a):
        if not torch.is_tensor(a):
            return a
        alive.append(a)
        return tuple(a.shape), str(a.dtype), ids.setdefault((a.untyped_storage().data_ptr(), a.storage_offset()), len(ids))

    def call(name, *args, **kwargs):
        if kwargs:                   # the complete tuple: what the same launch written without keywords records
            args = _lib.bind_args(name, args, kwargs)
        rec.launches.append((name,) + tuple(arg(a) for a in args))

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
    digest, count = sweep()
    print('%s  %d configurations  %s' % (digest, count, os.path.abspath(tree)))
