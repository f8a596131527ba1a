"""The decoder's two-valued data gradient from stored sign bits (tvae_linear_dgrad_x6 with vg_bits: dense_x6_kernel<5, NP, EPI>
in its three epilogue instances, the bits-only row sums and dWo from the weight-gradient identity) against the float64
statement of tests/dense_bits_ref.py.  The bit WORDS are drawn directly as random int32 (no forward pass), aux decides its mask
on the very fp32 values the kernel reads, and the recomputed first layer is drawn on a 1/64 grid in [-4, 4] so that its
pre-activation is exact in fp32 in any evaluation order (|pre| <= 40, a multiple of 2^-12: 18 significant bits) -- so no
element sits at zero to rounding, nothing is excluded and every arithmetic is held to its plain bound.

Names as in include/tvae_hip.h: M = rows of H = the reduction (16-row steps), K = rows of dX (512-row tiles), N in 128-column
tiles.  There is no query for the instance a call took; which branch of dense_x6_route (csrc/abi_dense_x6.hpp) a case
satisfies, from the arguments alone:

  lean_in  <5, NP, 2>   K == 512, dX NULL, in_xr AND in_bc given, no add, mask LeakyReLU (the first `if` of the bits branch)
  store    <5, NP, 3>   K % 512 == 0, dX stored, aux given, no in_xr, no add, mask LeakyReLU (the second)
  generic  <5, NP, 0>   everything else: K = 300 (clamped output rows), add given, in_xr with the mask from aux (in_bc NULL), or
                        no mask at all (aux NULL makes the launch's mask ACT_NONE whatever `mask` says)

What each shape is for: CASES below.  Tolerances are the project's: GEMM_TOL['f32'] for what comes off the matrix pipe with parts
3 and 2, the bound of test_conv1_dft_bf16_mode for parts 1, TOL for the fp32 sums (csum, row sums) in every arithmetic.
Observed on an MI355X, worst over all cases: 3.9e-7 with parts 3 and 2, 2.9e-3 with parts 1, 2.5e-7 for the fp32 sums -- a
factor of 50 inside the bounds, so an error of 1e-4 of a tensor fails.  Each of four arithmetic-only edits of the kernel (bit
position + 1 in the operand build; slope * csum dropped from the lean fused epilogue; 1 - slope -> 1 in the lean store
epilogue; the second column half left out of the row-sum write-out) failed every case of the instance it touches."""
import pytest
import torch

import dense_bits_ref as R
import guardband
from conftest import rel_err

pytestmark = pytest.mark.gpu
SLOPE = R.SLOPE
TOL = 2e-5                        # tests/test_hip_primitives.py
GEMM_TOL = {'f32': 2e-5}          # tests/test_hip_primitives.py
BF16_TOL = 1.5e-2                 # one-part mode: the bound of test_conv1_dft_bf16_mode
NAN = float('nan')


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in tests/test_hip_primitives.py: every call runs on relocated tensors between guard bands, twice."""
    with guardband.GuardedCalls(replay=True):
        yield


def dev():
    return torch.device('cuda:0')


def call(*a, **kw):
    from tvae._lib import call as c
    return c(*a, **kw)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def grid64(*shape, seed=0):
    """Integer multiples of 1/64 in [-4, 4]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-256, 257, shape, generator=g).float() / 64


def nans(*shape):
    return torch.full(shape, NAN, device=dev())


def same_words(a, b):
    """torch.equal on the bit patterns (NaN words that were left alone compare equal)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def planted_bits(M, N, seed):
    """Random words with an all-zero row, an all-ones row and rows whose words alternate 0x80000000 / 0x00000001 (both phases):
    only column 31, then only column 0 -- a bit position that is off by one, or a word taken from the neighbour, shows there."""
    words, _ = R.random_bits(M, N, seed)
    alt = torch.tensor([-2 ** 31, 1], dtype=torch.int32).repeat((N // 32 + 1) // 2)[:N // 32]
    words[0], words[1], words[2] = 0, -1, alt
    if M > 3:
        words[M - 1] = alt.roll(1) if N // 32 > 1 else 1
    return words, R.unpack(words)


def planted_aux(K, ld, seed):
    """Random fp32 with exact +0.0 and -0.0 planted (both take the slope: the mask is `> 0`)."""
    aux = rnd(K, ld, seed=seed)
    for i, (k, n) in enumerate([(0, 0), (K - 1, 5), (K // 2, 31), (K // 3, 32), (1, 127), (K - 2, 64)]):
        aux[k, n] = 0.0 if i % 2 == 0 else -0.0
    return aux


def first_layer(K, N, Np, lb, seed):
    """(xr, wc, bc, lb) on the 1/64 grid and the fp64 pre-activation; asserts that fp32 evaluates it exactly."""
    xr, wc, bc = grid64(N, 2, seed=seed), grid64(K, 2, seed=seed + 1), grid64(K, seed=seed + 2)
    LB = grid64(N // Np, K, seed=seed + 3) if lb else None
    pre = R.first_layer_pre(xr, wc, bc, LB, Np)
    p32 = wc[:, 1:2] * xr[:, 1][None, :] + (wc[:, 0:1] * xr[:, 0][None, :] + bc[:, None])
    if lb:
        p32 = p32 + LB[torch.arange(N) // Np].t()
    assert p32.dtype == torch.float32 and torch.equal(p32.double(), pre)
    return xr, wc, bc, LB, pre


# kind, M, K, N, options: pad (ldx = N + pad), fuse ('pre': in-tail with the recomputed mask, 'aux': with the mask from aux),
# Np, lb, aux, add, store (dX given), bias (rs_bias given), amax (y_amax for parts 3 and 2, and a second run without it)
CASES = [
    # lean fused instance <5, *, 2>
    ('lean_in', 512, 512, 1024, dict(fuse='pre', Np=256, lb=True, bias=True)),       # the hot shape, small
    ('lean_in', 384, 512, 1152, dict(fuse='pre', Np=128, lb=True, bias=True)),       # 9 column tiles: the ninth on the second XCD
    #                                                                                  group of the packed map; a new image per tile
    ('lean_in', 200, 512, 384, dict(fuse='pre', Np=384, lb=False, bias=True)),       # 200 = 12 * 16 + 8: clamped bit rows; in_lb NULL
    ('lean_in', 16, 512, 128, dict(fuse='pre', Np=128, lb=True, bias=False)),        # one step: the clamped prologue (nk > 1 ? 1 : 0)
    ('lean_in', 48, 512, 128, dict(fuse='pre', Np=128, lb=True, bias=True)),         # three steps: odd trip count of the unrolled loop
    # lean store <5, *, 3>
    ('store', 512, 512, 1024, dict(aux=True, store=True, pad=64, bias=True)),        # the row stride of a padded decoder buffer
    ('store', 320, 1024, 8320, dict(aux=True, store=True, bias=False, amax=True)),   # two row tiles, 65 column tiles (second 64-group)
    # generic <5, *, 0>
    ('generic', 512, 300, 640, dict(aux=True, add=True, store=True, bias=True)),     # clamped output rows
    ('generic', 300, 300, 512, dict(fuse='pre', Np=256, lb=True, bias=False)),       # the F = 300 decoder, dX NULL
    ('generic', 512, 512, 384, dict(fuse='aux', Np=128, aux=True, store=True, bias=True)),   # in_bc NULL: not the lean instance
    ('generic', 512, 1024, 256, dict(store=True, bias=True)),                        # aux NULL: no mask is applied
]


class Case:
    """Host inputs and the float64 reference of one shape (formed once, shared by the three arithmetics)."""

    def __init__(self, M, K, N, fuse=None, Np=0, lb=False, aux=False, add=False, store=False, pad=0, bias=True, amax=False,
                 bits=None, first=None):
        self.M, self.K, self.N, self.fuse, self.Np, self.store, self.ld, self.amax = M, K, N, fuse, Np, store, N + pad, amax
        self.W, self.wo, self.gy = rnd(M, K, seed=5, scale=M ** -0.5), rnd(M, seed=8), rnd(N, seed=9)
        self.rowdot, self.bias = rnd(M, seed=12), (rnd(M, seed=13) if bias else None)
        self.words, self.bits = planted_bits(M, N, seed=10) if bits is None else bits
        self.aux = planted_aux(K, self.ld, seed=6) if aux else None
        self.add = rnd(K, self.ld, seed=7) if add else None
        self.xr = self.wc = self.bc = self.lb = None
        mask = R.lrelu_mask(self.aux[:, :N]) if aux else None
        if fuse:
            self.xr, self.wc, bc, LB, pre = first_layer(K, N, Np, lb, seed=20) if first is None else first
            if fuse == 'pre':
                self.bc, self.lb, mask = bc, LB, R.lrelu_mask(pre)
        a = R.act_factor(self.bits)
        self.ref = {'csum': R.csum(self.W, self.wo)}
        dX = R.dgrad(self.W, self.wo, self.gy, a, mask=mask, add=self.add[:, :N] if add else None)
        if store:
            self.ref['dX'] = dX
        if fuse:
            for k_, v in zip(('gxr', 'part', 'Simg', 'dbc', 'dWc'), R.in_tail(dX, self.xr, self.wc, Np)):
                self.ref[k_] = v
        _, self.ref['rs_db'], self.ref['rs_dwo'] = R.row_sums(a, self.gy, self.wo, self.rowdot, self.bias)
        self.ref['rs_part'] = R.tile_sums(self.bits, self.gy)
        self.d = {k_: (getattr(self, k_).to(dev()) if getattr(self, k_) is not None else None)
                  for k_ in ('W', 'wo', 'gy', 'rowdot', 'bias', 'words', 'aux', 'add', 'xr', 'wc', 'bc', 'lb')}
        self.d['gysum'] = self.gy.sum().reshape(1).to(dev())                 # the fp32 sum of gy

    def cells(self, parts):
        """The split of W^T diag(wo) (transpose = 1, scale = wo) and its row sums."""
        from tvae._lib import query
        w3t = torch.empty(query('tvae_dense_x6_bytes', self.K, self.M) // 4, device=dev())
        csum = nans(self.K)
        call('tvae_dense_split2h' if parts == 2 else 'tvae_dense_split3', self.d['W'], self.K, w3t, w3t.numel() * 4, self.K,
             self.M, 1, self.d['wo'], csum)
        return w3t, csum

    def launch(self, parts, cells, amax=None, fused_totals=True):
        """One tvae_linear_dgrad_x6 call on NaN-filled outputs (+ tvae_dec_in_total behind a fused in-tail)."""
        M, K, N, d = self.M, self.K, self.N, self.d
        w3t, csum = cells
        o = {'csum': csum, 'rs_part': nans(M, N // 128, 2), 'rs_db': nans(M), 'rs_dwo': nans(M)}
        if self.store:
            o['dX_full'] = nans(K, self.ld)
        if self.fuse:
            o['gxr'], o['part'] = nans(N, 2), nans(N // 128, K, 3)
        part = o.get('part')
        call('tvae_linear_dgrad_x6', w3t, None, d['add'], d['aux'], o.get('dX_full'), M, N, K, N, self.ld, 1, SLOPE,
             in_xr=d['xr'], in_wc=d['wc'], in_gxr=o.get('gxr'), in_part=part, in_part_floats=part.numel() if self.fuse else 0,
             vg_gy=d['gy'], vg_csum=csum, in_bc=d['bc'], in_lb=d['lb'], in_np=self.Np, rs_part=o['rs_part'],
             rs_part_floats=o['rs_part'].numel(), rs_wo=d['wo'], rs_gysum=d['gysum'],
             rs_db=o['rs_db'] if fused_totals else None, rs_dwo=o['rs_dwo'] if fused_totals else None, parts=parts,
             vg_bits=d['words'], rs_rowdot=d['rowdot'], rs_bias=d['bias'], y_amax=amax)
        if self.store:
            o['dX'] = o['dX_full'][:, :N]
        if self.fuse:
            B = N // self.Np
            o['Simg'], o['dbc'], o['dWc'] = nans(B, K), nans(K), nans(K, 2)
            total_in = o['part'].clone()                                     # (tvae_dec_in_total consumes its input)
            call('tvae_dec_in_total', total_in, B, self.Np // 128, K, o['Simg'], o['dbc'], o['dWc'])
        return o

    def check(self, o, parts, label):
        """Every output finite and within its bound of the reference; prints the observed errors."""
        gemm = GEMM_TOL['f32'] if parts > 1 else BF16_TOL
        errs, bad = [], []
        for k_, ref in self.ref.items():
            got = o[k_][:, :, 0] if k_ == 'rs_part' else o[k_]
            tol = TOL if k_ in ('csum', 'rs_part', 'rs_db', 'rs_dwo') else gemm
            e = rel_err(got, ref) if bool(torch.isfinite(got).all()) else float('inf')
            errs.append('%s %.3g' % (k_, e))
            if not e < tol:
                bad.append((k_, e, tol))
        print('%s M %d K %d N %d parts %d: rel_err %s' % (label, self.M, self.K, self.N, parts, ', '.join(errs)))
        assert not bad, (label, parts, bad)
        assert bool(torch.isnan(o['rs_part'][:, :, 1]).all())                # the bits form writes only the first word of a pair
        if self.store and self.ld > self.N:
            assert bool(torch.isnan(o['dX_full'][:, self.N:]).all())         # the pad columns of the row stride stay untouched


@pytest.mark.parametrize('kind,M,K,N,opt', CASES, ids=['%s-M%d-K%d-N%d' % c[:4] for c in CASES])
def test_dgrad_from_bits_against_fp64(kind, M, K, N, opt):
    c = Case(M, K, N, **opt)
    for parts in (3, 2, 1):
        cells = c.cells(parts)
        amax = torch.zeros(1, device=dev()) if (c.amax and parts > 1) else None
        o = c.launch(parts, cells, amax=amax)
        c.check(o, parts, kind)
        if amax is not None:
            assert float(amax) == float(o['dX'].abs().max())                 # exactly the maximum of what was stored
            o2 = c.launch(parts, cells)
            assert torch.equal(o2['dX'], o['dX'])


def test_dgrad_from_bits_row_sum_totals_257_tiles():
    """257 column tiles: more than the 256 threads of dgrad_rowsum_total_kernel, so its loop over a row's tiles takes a second
    trip.  Fused totals against rs_db = rs_dwo = NULL followed by tvae_dgrad_rowsum_total with rowdot and bias: bit for bit the
    same, and both against float64.  (K = 512 with aux and a stored dX: the lean store instance.)"""
    M, K, N = 64, 512, 257 * 128
    c = Case(M, K, N, aux=True, store=True, bias=True)
    for parts in (3, 2, 1):
        cells = c.cells(parts)
        a = c.launch(parts, cells)
        b = c.launch(parts, cells, fused_totals=False)
        assert bool(torch.isnan(b['rs_db']).all()) and bool(torch.isnan(b['rs_dwo']).all())
        call('tvae_dgrad_rowsum_total', b['rs_part'], N // 128, M, c.d['wo'], c.d['gysum'], SLOPE, b['rs_db'], b['rs_dwo'],
             c.d['rowdot'], c.d['bias'])
        for k_ in ('dX', 'rs_part', 'rs_db', 'rs_dwo'):
            assert same_words(a[k_], b[k_]), (parts, k_)
        c.check(a, parts, 'totals-fused')
        c.check(b, parts, 'totals-split')


def test_dgrad_from_bits_chained_with_real_bits():
    """Forward, weight gradient and data gradient of one decoder tail chained through the bits the forward stores (F = M = K =
    512, B = 2, Np = 256): tvae_linear_fwd_x6 with the recomputed first layer, Y = NULL, the fused output dot and sign_bits;
    tvae_linear_wgrad_x6 from those bits with rd_w / rd_rowdot; tvae_linear_dgrad_x6 from the bits, that rowdot and the layer's
    bias.  The device's bits, unpacked on the host, are the reference's `a`, so dX / gxr / part / rs_db / dW are held to the
    plain bounds; rs_dwo goes against the TRUE float64 sum_n gy[n] H[m][n], and at most 2 bits may disagree with H64 > 0 (the
    bound of test_h3_decoder_entry_points for elements at zero to rounding; in float64 itself no |pre| of these seeds is below
    1e-6, asserted).  Parts 3 and 2 only: with one bf16 part the forward's own error flips signs by the hundred and rowdot
    comes off the matrix pipe at 1.5e-2, so neither the bit bound nor TOL on rs_dwo applies to it."""
    from tvae._lib import query
    M = K = 512
    B, Np = 2, 256
    N = B * Np
    first = first_layer(K, N, Np, True, seed=20)
    xr, wc, bc, LB, pre0 = first
    H0 = torch.where(pre0 > 0, pre0, SLOPE * pre0)
    W, b = rnd(M, K, seed=5, scale=K ** -0.5), rnd(M, seed=13)
    wo, gy, cb = rnd(M, seed=8), rnd(N, seed=9), rnd(1, seed=14)
    pre = W.double() @ H0 + b.double()[:, None]
    assert float(pre.abs().min()) >= 1e-6
    H = torch.where(pre > 0, pre, 0.01 * pre)
    d = {k_: v.to(dev()) for k_, v in dict(xr=xr, wc=wc, bc=bc, lb=LB, W=W, b=b, wo=wo, gy=gy, cb=cb).items()}
    va = dict(va_xr=d['xr'], va_wc=d['wc'], va_bc=d['bc'], va_lb=d['lb'], va_np=Np)
    for parts in (3, 2):
        split = 'tvae_dense_split2h' if parts == 2 else 'tvae_dense_split3'
        w3 = torch.empty(query('tvae_dense_x6_bytes', M, K) // 4, device=dev())
        call(split, d['W'], K, w3, w3.numel() * 4, M, K, 0, None, None)
        words = torch.zeros(M, N // 32, dtype=torch.int32, device=dev())
        col_y = nans(N)
        call('tvae_linear_fwd_x6', w3, None, d['b'], None, None, M, N, K, N, N, 1, SLOPE, col_w=d['wo'], col_b=d['cb'],
             col_y=col_y, **va, sign_bits=words, parts=parts)
        ws = torch.empty(query('tvae_linear_wgrad_x6_ws_floats', M, N, K), device=dev())
        dW, rowdot = nans(M, K), nans(M)
        call('tvae_linear_wgrad_x6', None, None, dW, ws, ws.numel(), M, N, K, N, N, 0, vg_wo=d['wo'], vg_gy=d['gy'], vg_act=1,
             vg_slope=SLOPE, **va, vg_bits=words, parts=parts, rd_w=d['W'], rd_ldw=K, rd_rowdot=rowdot)
        host_words = words.cpu()
        bits = R.unpack(host_words)
        flips = int((bits != (pre > 0)).sum())
        c = Case(M, K, N, fuse='pre', Np=Np, lb=True, bits=(host_words, bits), first=first)
        assert torch.equal(c.W, W) and torch.equal(c.wo, wo) and torch.equal(c.gy, gy)             # (the same seeds)
        c.d['rowdot'], c.d['bias'] = rowdot, d['b']                          # the weight gradient's rowdot, the layer's bias
        a = R.act_factor(bits)
        G = (gy.double()[None, :] * a) @ H0.t()
        _, c.ref['rs_db'], _ = R.row_sums(a, gy, wo, (W.double() * G).sum(1), b)
        c.ref['rs_dwo'] = H @ gy.double()
        o = c.launch(parts, c.cells(parts))
        e_y, e_dw = rel_err(col_y, wo.double() @ H + cb.double()), rel_err(dW, wo.double()[:, None] * G)
        e_rd = rel_err(rowdot, (W.double() * G).sum(1))
        print('chained parts %d: bit flips %d, rel_err col_y %.3g dW %.3g rowdot %.3g' % (parts, flips, e_y, e_dw, e_rd))
        c.check(o, parts, 'chained')
        assert flips <= 2
        assert torch.isfinite(dW).all() and torch.isfinite(rowdot).all() and torch.isfinite(col_y).all()
        assert e_y < GEMM_TOL['f32'] and e_dw < GEMM_TOL['f32'] and e_rd < GEMM_TOL['f32']


def test_dgrad_from_bits_refusals():
    """Argument combinations the bits form must refuse: each raises and leaves every NaN-filled output all NaN (the guard bands
    check the same of every other tensor of the call)."""
    from tvae._lib import query
    M, K, N, Np = 32, 64, 384, 128
    xr, wc, bc, LB, _ = first_layer(K, N, Np, True, seed=20)

    def setup(M):
        W, wo, gy = rnd(M, K, seed=5, scale=M ** -0.5).to(dev()), rnd(M, seed=8).to(dev()), rnd(N, seed=9).to(dev())
        w3t = torch.empty(query('tvae_dense_x6_bytes', K, M) // 4, device=dev())
        csum = torch.empty(K, device=dev())
        call('tvae_dense_split3', W, K, w3t, w3t.numel() * 4, K, M, 1, wo, csum)
        return dict(w3t=w3t, dpre=None, add=None, aux=planted_aux(K, N, seed=6).to(dev()), dX=nans(K, N), M=M, N=N, K=K, ldd=N, ldx=N,
                    mask=1, slope=SLOPE, in_xr=None, in_wc=None, in_gxr=None, in_part=None, in_part_floats=0, vg_wo=None, vg_gy=gy,
                    vg_csum=csum, in_bc=None, in_lb=None, in_np=0, rs_part=nans(M, N // 128, 2), rs_part_floats=M * (N // 128) * 2,
                    rs_wo=wo, rs_gysum=gy.sum().reshape(1), rs_db=nans(M), rs_dwo=nans(M), parts=3,
                    vg_bits=planted_bits(M, N, seed=10)[0].to(dev()), rs_rowdot=rnd(M, seed=12).to(dev()),
                    rs_bias=rnd(M, seed=13).to(dev()), x_amax=None, y_amax=None)

    outputs = ('dX', 'in_gxr', 'in_part', 'rs_part', 'rs_db', 'rs_dwo')

    def refused(a, **change):
        a = dict(a, **change)
        for k_ in outputs:
            if a[k_] is not None:
                a[k_].fill_(NAN)
        with pytest.raises(Exception):
            call('tvae_linear_dgrad_x6', **a)
        for k_ in outputs:
            assert a[k_] is None or bool(torch.isnan(a[k_]).all()), k_

    base = setup(M)
    call('tvae_linear_dgrad_x6', **base)                                     # the unchanged arguments are a valid call
    assert all(bool(torch.isfinite(base[k_]).all()) for k_ in ('dX', 'rs_db', 'rs_dwo'))
    intail = dict(in_xr=xr.to(dev()), in_wc=wc.to(dev()), in_gxr=nans(N, 2), in_part=nans(N // 128, K, 3),
                  in_part_floats=(N // 128) * K * 3, in_bc=bc.to(dev()), in_lb=LB.to(dev()), in_np=Np, aux=None)
    fused = dict(base, **intail)
    call('tvae_linear_dgrad_x6', **fused)                                    # ... and so is the fused form that in_np = 96 changes
    assert all(bool(torch.isfinite(fused[k_]).all()) for k_ in ('dX', 'in_gxr', 'in_part'))
    refused(base, vg_csum=None)                                              # vg_bits without vg_csum
    refused(base, rs_part=None, rs_part_floats=0)                            # vg_bits without rs_part
    refused(base, rs_rowdot=None)                                            # vg_bits with rs_db but no rs_rowdot
    refused(base, vg_bits=None, dpre=rnd(M, N, seed=2).to(dev()))            # rs_rowdot without vg_bits (H itself as the operand)
    refused(base, mask=2)                                                    # the two-valued form exists for LeakyReLU only
    refused(setup(528))                                                      # M = 528 > 512: the row sums live in one 512-row table
    refused(base, rs_part_floats=base['rs_part_floats'] - 1)                 # rs_part one float short
    refused(fused, in_np=96)                                                 # in_bc with panels that straddle images
