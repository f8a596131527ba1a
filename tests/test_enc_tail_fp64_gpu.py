"""The encoder tail (conv2 1x1x1 + the stacked head projection) through its C-ABI entry points -- tvae_enc_tail_fwd_x6 /
_dgrad_x6 / _wgrad_x6, tvae_enc_tail_fwd_wide / _dgrad_wide / _wgrad_wide and the slab total behind both weight gradients --
against tests/enc_tail_ref.py in float64, one case for every branch (case lists and what each reaches: enc_tail_ref.py;
tests/test_enc_tail_ref_cpu.py proves the branch arithmetic of the lists for 256 and 304 CUs).

EVERY element of every output against K UNIT[parts] (condition quantity) + floor (K, UNIT and the floors of the h3 scales:
enc_tail_ref's docstring; K comes from CPU arithmetic, never from these kernels).  Strided inputs carry 1e30 in their pad
columns, strided outputs are prefilled with a sentinel that has to come back untouched, sign-word outputs with 0xA5A5A5A5:
every word of a column < N has to equal `value > 0` of the STORED tensor bit for bit (H: the kernel's own; A1: the input),
every word behind N the prefill.  The data and weight gradients take PLANTED sign words (random, all zero, all one, a walking
one and its complement), never the forward's.  Refusals are exact: an error, and every output still holds its prefill.
Every call runs between guard bands, twice (replay).

Worst ratio seen on an MI355X, by output: enc_tail_ref.GPU_SEEN; test_worst_ratios prints this run's.

One-line changes to the kernels, each built and run once (tests of test_hip_primitives.py / test_midsize_kernels.py that select
`enc_tail`: 29; this file: 320).  Earlier tests failing | tests of this file failing:
  et_split<3> leaving the third bf16 part zero                                     0 | 56  (the single-product rows and columns)
  x6 data gradient masking with wAsn, the NEXT chunk's words of A1                 4 |  7  (only where a wave runs two chunks)
  the forward's head-row store taking ve / vo swapped for q = 1                    8 | 55
  the wide partial k-step clamping rows with rem instead of rem - 1            4 + 1 | 30 + 26 (+: guard-band reports; wide tests only)
  ia_sm[et_row(i, r, 0)] in the x6 forward's h3 epilogue (lane half dropped)      11 | 34
  the x6 data gradient's h3 chunk scale gs taken once before the chunk loop        0 |  3  (the 2^20 chunk among the second chunks)
  hb[i] <<= 4 * kh applied after the shuffle                                      11 | 44
  wgrad_x6's h3 scale of dH without the row-sum factor sum_h |Wh[h][row]|          2 | 13  (the column of Wh that is 4)"""
import math

import pytest
import torch

import enc_tail_ref as R
import guardband

pytestmark = pytest.mark.gpu
WORST = {}
NAN = float('nan')
C = R.C
SLOPE = 0.01


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in test_hip_primitives.py: every C-ABI call on relocated tensors between guard bands, twice from the same inputs."""
    with guardband.GuardedCalls(replay=True):
        yield


def dev():
    return torch.device('cuda:0')


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def call(*a, **kw):
    from tvae._lib import call as c
    return c(*a, **kw)


def query(*a):
    from tvae._lib import query as q
    return q(*a)


def G(t):
    return None if t is None else t.contiguous().to(dev())


def strided(T, ld, fill=R.PAD_IN):
    """T [rows][N] as the leading columns of a [rows][ld] device tensor whose pad columns hold `fill`."""
    out = torch.full((T.shape[0], ld), fill, device=dev())
    out[:, :T.shape[1]] = T.to(dev())
    return out


def full(shape, v=R.SENTINEL):
    return torch.full(shape, v, device=dev())


def words(N, extra=3):
    """a sign-word output [N + extra][4], prefilled"""
    return torch.full((N + extra, 4), R.BITS_PREFILL, dtype=torch.int32, device=dev())


def check(name, parts, got, ref, cond, floor=None, what=None):
    r = R.ratio(got, ref, cond, R.UNIT[parts], floor)
    WORST[name, parts] = max(WORST.get((name, parts), 0.0), r)
    print(f'{name} parts {parts} {"" if what is None else what}: ratio {r:.3f} of K = {R.K[name]}')
    assert math.isfinite(r) and r <= R.K[name], (name, parts, what, r, R.K[name])


def pads_untouched(T, N):
    assert bool((T[:, N:] == R.SENTINEL).all()), 'pad columns of a strided output were written'


def check_words(got, N, stored, what):
    """got [N + extra][4] int32 after the call; stored [128][>= N]: the tensor whose signs the words describe"""
    want = R.pack(stored[:, :N] > 0)
    assert torch.equal(got[:N], want), (what, 'sign words differ from value > 0 of the stored tensor')
    assert bool((got[N:] == R.BITS_PREFILL).all()), (what, 'words of columns >= N were written')


def cells(W, rows, K, transpose, parts):
    """cells of W [.][ldw]: tvae_dense_split2h (parts = 2) or tvae_dense_split3 (3; 1 uses its first part)"""
    a3 = torch.zeros(query('tvae_dense_x6_bytes', rows, K) // 4, device=dev())
    W = G(W)
    call('tvae_dense_split2h' if parts == 2 else 'tvae_dense_split3', W, W.shape[1], a3, a3.numel() * 4, rows, K, transpose, None, None)
    return a3


REFS = {}


def shared(key, make):
    """a reference computed once and left unchanged"""
    if key not in REFS:
        REFS[key] = make()
    return REFS[key]


# ---- forward, both families ---------------------------------------------------------------------------------------------------
def run_fwd(wide, N, nh, act, has_b2, parts, scale=1.0, slack=1.0, dyn=False, on_gpu=False):
    fam = 'wide' if wide else 'x6'
    W2, b2, Wh, bh = R.weights(nh, dyn)
    b2 = b2 if has_b2 else None
    A1 = R.a1_case(N, scale, dyn)
    lda, ldh, ldo = N + R.PADS[0], N + R.PADS[1], N + R.PADS[2]
    A1s, H, heads = strided(A1, lda), full((C, ldh)), full((nh, ldo))
    bits_h, bits_a = (words(N), words(N)) if act == 1 else (None, None)
    amax = G(A1.abs().amax(1) * slack) if parts == 2 else None
    w3 = cells(W2, C, C, 0, parts)
    if wide:
        whp = cells(Wh[:, R.perm()], nh, C, 0, parts)
        args = ('tvae_enc_tail_fwd_wide', w3, whp, A1s, lda, G(b2), G(bh), nh)
    else:
        args = ('tvae_enc_tail_fwd_x6', w3, A1s, lda, G(b2), G(Wh), G(bh), nh)
    call(*args, H, ldh, heads, ldo, bits_h, bits_a, C, N, act, SLOPE, parts, amax)
    to = (lambda t: None if t is None else t.to(dev())) if on_gpu else (lambda t: t)
    w2_, a1_, b2_, wh_, bh_ = to(W2), to(A1), to(b2), to(Wh), to(bh)
    ref, cond = shared(('fwd', N, nh, act, has_b2, scale, dyn), lambda: R.both(R.fwd, w2_, a1_, b2_, wh_, bh_, act))
    floor = R.fwd_floor(wide, w2_, a1_, wh_, to(A1.abs().amax(1) * slack), ref['H']) if parts == 2 else {'H': None, 'heads': None}
    what = (N, nh, act, has_b2, scale, slack, dyn)
    check(f'{fam}_H', parts, H[:, :N], ref['H'], cond['H'], floor['H'], what)
    check(f'{fam}_heads', parts, heads[:, :N], ref['heads'], cond['heads'], floor['heads'], what)
    pads_untouched(H, N)
    pads_untouched(heads, N)
    zc = R.zero_column(N)
    if zc is not None:                                       # an all-zero column: H is exactly +0 where b2 is zero (or NULL)
        rows = R.ZERO_B_ROWS if has_b2 else list(range(C))
        hz = H[rows, zc]
        assert bool((hz == 0).all()) and not bool(torch.signbit(hz).any()), 'H of an all-zero column with b2 = 0 is not +0'
    if act == 1:
        check_words(bits_h, N, H, (fam, 'bits_h') + what)
        check_words(bits_a, N, A1.to(dev()), (fam, 'bits_a') + what)
    # H == NULL (inference): no H, no sign words, the same head rows bit for bit
    h2 = full((nh, ldo))
    call(*args, None, ldh, h2, ldo, None, None, C, N, act, SLOPE, parts, amax)
    assert torch.equal(h2, heads), 'the inference-mode head rows differ from the training call'


@pytest.mark.parametrize('parts', [3, 2, 1])
@pytest.mark.parametrize('N,nh,act,has_b2', R.x6_fwd_cases())
def test_x6_fwd(N, nh, act, has_b2, parts):
    run_fwd(False, N, nh, act, has_b2, parts)


@pytest.mark.parametrize('scale,slack,dyn,act', R.h3_fwd_variants())
def test_x6_fwd_h3_scales(scale, slack, dyn, act):
    """h3: amax_a1 exact and 64 x loose, a channel of A1 and a row of W2 2^-20 below the rest, activations of size 1, 1e-5, 1e3"""
    run_fwd(False, 257, 7, act, True, 2, scale, slack, dyn)


@pytest.mark.parametrize('parts', [2, 1])
@pytest.mark.parametrize('N,nh,act,has_b2', R.wide_fwd_cases())
def test_wide_fwd(N, nh, act, has_b2, parts):
    run_fwd(True, N, nh, act, has_b2, parts)


@pytest.mark.parametrize('wide,parts', [(False, 3), (False, 2), (False, 1), (True, 2), (True, 1)])
@pytest.mark.parametrize('which', [0, 1])
def test_fwd_persistent_grid(which, wide, parts):
    """More chunks than waves: waves with unequal chunk counts, the clamped reload, a ragged chunk as a wave's second."""
    run_fwd(wide, R.ns_big(cus())[which], 103 if wide else 7, 1, True, parts, on_gpu=True)


# ---- data gradient from planted sign words ------------------------------------------------------------------------------------
def run_dgrad(wide, N, nh, pat, parts, slack=1.0, big=False):
    fam = 'wide' if wide else 'x6'
    W2, _, Wh, _ = R.weights(nh)
    d = R.dheads_case(nh, N, cus() if big else None)
    bh_, ba_ = R.bit_pattern(pat, N, 1), R.bit_pattern(pat, N, 2)
    ldd, lda, ldh = N + R.PADS[3], N + R.PADS[0], N + R.PADS[1]
    ds, dA1 = strided(d, ldd), full((C, lda))
    wH, wA = G(R.pack(bh_)), G(R.pack(ba_))
    w3p = cells(W2.t()[:, R.perm()], C, C, 0, parts)
    to = (lambda t: t.to(dev())) if big else (lambda t: t)
    w2_, wh_, d_, bh__, ba__ = to(W2), to(Wh), to(d), to(bh_), to(ba_)
    ref, cond = shared(('dgrad', N, nh, pat, big), lambda: R.both(R.dgrad, w2_, wh_, d_, bh__, ba__))
    amax_d = d.abs().max() * slack
    floor = R.dgrad_floor(wide, w2_, wh_, d_, bh__, ba__, to(amax_d), ref) if parts == 2 else {'dH': None, 'dA1': None}
    what = (N, nh, pat, slack)
    if wide:
        wht = cells(Wh, C, nh, 1, parts)
        am = G(amax_d.reshape(1)) if parts == 2 else None
        dH = full((C, ldh))
        call('tvae_enc_tail_dgrad_wide', wht, w3p, ds, ldd, nh, wH, wA, dH, ldh, dA1, lda, C, N, SLOPE, parts, am)
        check('wide_dH', parts, dH[:, :N], ref['dH'], cond['dH'], floor['dH'], what)
        pads_untouched(dH, N)
        dA2 = full((C, lda))                                   # dH == NULL: the same dA1 bit for bit
        call('tvae_enc_tail_dgrad_wide', wht, w3p, ds, ldd, nh, wH, wA, None, ldh, dA2, lda, C, N, SLOPE, parts, am)
        assert torch.equal(dA2, dA1), 'dA1 without the dH output differs from the call that stores dH'
    else:
        wh3 = cells(Wh, C, nh, 1, 3)                           # the skinny GEMM's cells are the exact split in every arithmetic
        call('tvae_enc_tail_dgrad_x6', w3p, wh3, ds, ldd, nh, wH, wA, dA1, lda, C, N, SLOPE, parts)
    check(f'{fam}_dA1', parts, dA1[:, :N], ref['dA1'], cond['dA1'], floor['dA1'], what)
    pads_untouched(dA1, N)
    for ch, f in R.special_chunks(N, cus() if big else None).items():
        if f == 0.0:                                         # a chunk of dheads exactly zero: exactly +-0 out
            assert bool((dA1[:, 32 * ch:min(N, 32 * ch + 32)] == 0).all()), 'the zero chunk of dheads gave non-zero dA1'


@pytest.mark.parametrize('parts', [3, 2, 1])
@pytest.mark.parametrize('N,nh,pat', R.x6_dgrad_cases())
def test_x6_dgrad(N, nh, pat, parts):
    run_dgrad(False, N, nh, pat, parts)


@pytest.mark.parametrize('parts', [2, 1])
@pytest.mark.parametrize('N,nh,pat,slack', R.wide_dgrad_cases())
def test_wide_dgrad(N, nh, pat, slack, parts):
    run_dgrad(True, N, nh, pat, parts, slack)


@pytest.mark.parametrize('wide,parts', [(False, 3), (False, 2), (False, 1), (True, 2), (True, 1)])
@pytest.mark.parametrize('which', [0, 1])
def test_dgrad_persistent_grid(which, wide, parts):
    """More chunks than waves: the hand-over of the next chunk's sign words, the two-ahead loads, a chunk scale per chunk (a
    chunk 2^20 above its neighbours among the SECOND chunks of the waves)."""
    run_dgrad(wide, R.ns_big(cus())[which], 103 if wide else 7, 'random', parts, big=True)


# ---- weight gradients ---------------------------------------------------------------------------------------------------------
def both_totals(monkeypatch, run):
    """run() under both settings of TVAE_MIDSIZE_ILP (read at every call): the slab totals add in the same order, bit for bit"""
    out = []
    for v in ('0', '1'):
        monkeypatch.setenv('TVAE_MIDSIZE_ILP', v)
        out.append(run())
    assert torch.equal(out[0], out[1]), 'the two slab-total kernels differ'
    return out[0]


PAD_GARBAGE = (1e30, -3.0)          # behind row rows_d of the D buffer, in two calls


def wgrad_chunk_cases():
    return [(i, (0, 4, 64)[i % 3]) for i in range(6)]          # (index into wgrad_chunks(cus), pad of lda / ldd)


@pytest.mark.parametrize('parts', [3, 2, 1])
@pytest.mark.parametrize('nh', R.WGRAD_X6_NH)
@pytest.mark.parametrize('ci,pad', wgrad_chunk_cases())
def test_x6_wgrad(ci, pad, nh, parts, monkeypatch):
    N = 32 * R.wgrad_chunks(cus())[ci]
    Wh = R.wgrad_wh(nh)
    A, _ = R.wgrad_case(N)
    d = R.dheads_case(nh, N, plain=True)
    pat = R.BIT_PATTERNS[(ci + nh) % 5]
    bits = R.bit_pattern(pat, N, 1)
    ld = N + pad
    As, ds, wH, Whd = strided(A, ld), strided(d, ld), G(R.pack(bits)), G(Wh)
    amax = G(A.abs().amax(1)) if parts == 2 else None
    nws = query('tvae_enc_tail_wgrad_x6_ws_floats', N)

    def run():
        ws, dW2 = full((nws,), NAN), full((C, C), NAN)
        call('tvae_enc_tail_wgrad_x6', As, ld, ds, ld, nh, wH, Whd, dW2, ws, nws, C, N, SLOPE, parts, amax)
        return dW2
    dW2 = both_totals(monkeypatch, run)
    dH = R.mask(bits) * (Wh.double().t() @ d.double())
    cH = R.mask(bits) * (Wh.double().abs().t() @ d.double().abs())
    floor = R.wgrad_floor(dH, A, R.wgrad_x6_scale_d(Wh, d), A.abs().amax(1)) if parts == 2 else None
    check('x6_dW2', parts, dW2, R.wgrad(dH, A), R.wgrad(cH, A, cond=True), floor, (N, nh, pad, pat))


def test_x6_wgrad_h3_dynamic_range(monkeypatch):
    """h3: a channel of A1 and a head row 2^-20 below the rest, a column of Wh all zero (the bound of that row of dH is 0: its
    row of dW2 is exactly zero), amax_a1 64 x loose."""
    N, nh = 96, 7
    Wh = R.wgrad_wh(nh, True)
    Wh[:, 50] = 0.0
    A, _ = R.wgrad_case(N, True)
    d, bits = R.dheads_case(nh, N, plain=True), R.bit_pattern('random', N, 1)
    amax = A.abs().amax(1) * 64.0
    nws = query('tvae_enc_tail_wgrad_x6_ws_floats', N)

    def run():
        ws, dW2 = full((nws,), NAN), full((C, C), NAN)
        call('tvae_enc_tail_wgrad_x6', G(A), N, G(d), N, nh, G(R.pack(bits)), G(Wh), dW2, ws, nws, C, N, SLOPE, 2, G(amax))
        return dW2
    dW2 = both_totals(monkeypatch, run)
    dH = R.mask(bits) * (Wh.double().t() @ d.double())
    cH = R.mask(bits) * (Wh.double().abs().t() @ d.double().abs())
    check('x6_dW2', 2, dW2, R.wgrad(dH, A), R.wgrad(cH, A, cond=True), R.wgrad_floor(dH, A, R.wgrad_x6_scale_d(Wh, d), amax), 'dyn')
    assert bool((dW2[50] == 0).all())


@pytest.mark.parametrize('rows_d', R.WGRAD_WIDE_ROWS)
@pytest.mark.parametrize('ci,pad', wgrad_chunk_cases())
def test_wide_wgrad(ci, pad, rows_d, monkeypatch):
    """Rows >= rows_d of dW are unspecified; rows < rows_d must not depend on what lies behind row rows_d of a larger D buffer."""
    N = 32 * R.wgrad_chunks(cus())[ci]
    dyn = (ci + rows_d) % 2 == 1
    A, D = R.wgrad_case(N, dyn)
    D = D[:rows_d]
    ld = N + pad
    slack = (1.0, 64.0)[ci % 2]
    am_d, am_a = D.abs().max() * slack, A.abs().amax(1) * slack
    As = strided(A, ld)
    nws = query('tvae_enc_tail_wgrad_x6_ws_floats', N)
    outs = []
    for garbage in (PAD_GARBAGE[0], PAD_GARBAGE[1]):
        Db = torch.full((rows_d + 3, ld), garbage, device=dev())
        Db[:rows_d] = strided(D, ld)

        def run():
            ws, dW = full((nws,), NAN), full((C, C), NAN)
            call('tvae_enc_tail_wgrad_wide', Db, ld, rows_d, As, ld, dW, ws, nws, C, N, G(am_d.reshape(1)), G(am_a))
            return dW[:rows_d].clone()
        outs.append(both_totals(monkeypatch, run))
    assert torch.equal(outs[0], outs[1]), 'rows < rows_d depend on what lies behind row rows_d'
    ref, cond = R.both(R.wgrad, D, A)
    check('wide_dW', 2, outs[0], ref, cond, R.wgrad_floor(D, A, am_d, am_a), (N, rows_d, pad, slack, dyn))


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refused(name, *args):
    with pytest.raises(Exception):
        call(name, *args)


def test_refusals_forward_and_data_gradient():
    N, nh = 64, 7
    W2, b2, Wh, bh = R.weights(nh)
    A1, d = G(R.a1_case(N)), G(R.dheads_case(nh, N))
    H, heads, dA1, dH = full((C, N)), full((nh, N)), full((C, N)), full((C, N))
    bits = [words(N, 1), words(N, 1)]
    given = [G(R.pack(R.bit_pattern('random', N, s))) for s in (1, 2)]
    am, amd = G(R.a1_case(N).abs().amax(1)), G(R.dheads_case(nh, N).abs().max().reshape(1))
    w3 = {p: cells(W2, C, C, 0, p) for p in (3, 2)}
    w3p = {p: cells(W2.t()[:, R.perm()], C, C, 0, p) for p in (3, 2)}
    wh3, whp, wht = cells(Wh, C, nh, 1, 3), cells(Wh[:, R.perm()], nh, C, 0, 2), cells(Wh, C, nh, 1, 2)
    b2d, Whd, bhd = G(b2), G(Wh), G(bh)
    BIG = 1 << 25

    def fx6(w=w3[3], a=A1, lda=N, nh_=nh, h=H, ldh=N, ldo=N, bh_=None, ba_=None, c=C, n=N, act=1, parts=3, amax=None):
        return ('tvae_enc_tail_fwd_x6', w, a, lda, b2d, Whd, bhd, nh_, h, ldh, heads, ldo, bh_, ba_, c, n, act, SLOPE, parts, amax)

    def fwide(w=w3[2], lda=N, nh_=nh, ldh=N, ldo=N, bh_=None, ba_=None, c=C, n=N, act=1, parts=2, amax=am):
        return ('tvae_enc_tail_fwd_wide', w, whp, A1, lda, b2d, bhd, nh_, H, ldh, heads, ldo, bh_, ba_, c, n, act, SLOPE, parts, amax)

    def dx6(w=w3p[3], ldd=N, nh_=nh, bh_=given[0], ba_=given[1], lda=N, c=C, n=N, parts=3):
        return ('tvae_enc_tail_dgrad_x6', w, wh3, d, ldd, nh_, bh_, ba_, dA1, lda, c, n, SLOPE, parts)

    def dwide(ldd=N, nh_=nh, bh_=given[0], ba_=given[1], ldh=N, lda=N, c=C, n=N, parts=2, amax=amd):
        return ('tvae_enc_tail_dgrad_wide', wht, w3p[2], d, ldd, nh_, bh_, ba_, dH, ldh, dA1, lda, c, n, SLOPE, parts, amax)

    off = torch.full((4 * N + 4,), R.BITS_PREFILL, dtype=torch.int32, device=dev())[1:]       # a word buffer 4 bytes off 16
    assert off.data_ptr() % 16 == 4
    cells_off = torch.cat([torch.zeros(1, device=dev()), w3[3]])[1:]
    assert cells_off.data_ptr() % 16 == 4
    for bad in (fx6(c=64), fx6(nh_=0), fx6(nh_=8), fx6(parts=2, w=w3[2]), fx6(parts=4), fx6(act=0, bh_=bits[0], ba_=bits[1]),
                fx6(act=2, bh_=bits[0], ba_=bits[1]), fx6(bh_=off, ba_=bits[1]), fx6(bh_=bits[0], ba_=off), fx6(w=cells_off),
                fx6(bh_=bits[0]), fx6(ba_=bits[1]),                          # sign words: both or neither
                fx6(lda=BIG), fx6(ldh=BIG), fx6(ldo=BIG),
                fwide(c=64), fwide(nh_=0), fwide(nh_=129), fwide(parts=3, w=w3[3]), fwide(amax=None),
                fwide(act=0, bh_=bits[0], ba_=bits[1]), fwide(bh_=bits[0]), fwide(ba_=bits[1]), fwide(bh_=off, ba_=bits[1]),
                fwide(lda=BIG), fwide(ldh=BIG), fwide(ldo=BIG),
                dx6(c=64), dx6(nh_=0), dx6(nh_=8), dx6(parts=0), dx6(bh_=None), dx6(ba_=None), dx6(bh_=off), dx6(ba_=off),
                dx6(w=cells_off), dx6(ldd=BIG), dx6(lda=BIG),
                dwide(c=64), dwide(nh_=0), dwide(nh_=129), dwide(parts=3), dwide(amax=None), dwide(bh_=None), dwide(ba_=off),
                dwide(ldd=BIG), dwide(ldh=BIG), dwide(lda=BIG)):
        refused(*bad)
    for t in (H, heads, dA1, dH):
        assert bool((t == R.SENTINEL).all())
    for t in bits:
        assert bool((t == R.BITS_PREFILL).all())
    for ok in (fx6(n=0), fwide(n=0), dx6(n=0), dwide(n=0)):       # N = 0: success, nothing touched
        call(*ok)
    for t in (H, heads, dA1, dH):
        assert bool((t == R.SENTINEL).all())


def test_refusals_weight_gradients():
    N, nh = 64, 7
    _, _, Wh, _ = R.weights(nh)
    A, D = R.wgrad_case(N)
    d = R.dheads_case(nh, N, plain=True)
    Ad, Dd, dd, Whd, wH = G(A), G(D), G(d), G(Wh), G(R.pack(R.bit_pattern('random', N, 1)))
    A68, d68 = strided(A, 68), strided(d, 68)
    nws = query('tvae_enc_tail_wgrad_x6_ws_floats', N)
    assert nws == min(N // 32, cus()) * C * C + 8
    ws, dW = full((nws,)), full((C, C))
    am_a, am_d = G(A.abs().amax(1)), G(D.abs().max().reshape(1))
    A_off = torch.cat([torch.zeros(1, device=dev()), Ad.reshape(-1)])[1:]
    assert A_off.data_ptr() % 16 == 4

    def wx6(a=Ad, lda=N, dh=dd, ldd=N, nh_=nh, b=wH, c=C, n=N, wsf=nws, parts=3, amax=None):
        return ('tvae_enc_tail_wgrad_x6', a, lda, dh, ldd, nh_, b, Whd, dW, ws, wsf, c, n, SLOPE, parts, amax)

    def wwide(dm=Dd, ldd=N, rows=103, a=Ad, lda=N, c=C, n=N, wsf=nws, amd=am_d, ama=am_a):
        return ('tvae_enc_tail_wgrad_wide', dm, ldd, rows, a, lda, dW, ws, wsf, c, n, amd, ama)

    for bad in (wx6(c=64), wx6(nh_=0), wx6(nh_=8), wx6(n=N - 1), wx6(a=A68, lda=67), wx6(dh=d68, ldd=66), wx6(wsf=nws - 1),
                wx6(parts=2), wx6(parts=4), wx6(b=None), wx6(a=A_off), wx6(lda=N - 4), wx6(ldd=N - 4),
                wwide(c=64), wwide(rows=0), wwide(rows=129), wwide(n=N - 1), wwide(a=A68, lda=67), wwide(lda=N - 4), wwide(ldd=N - 4),
                wwide(wsf=nws - 1), wwide(amd=None), wwide(ama=None), wwide(a=A_off)):
        refused(*bad)
    assert bool((ws == R.SENTINEL).all()) and bool((dW == R.SENTINEL).all())
    call(*wx6(n=0))
    call(*wwide(n=0))
    assert bool((ws == R.SENTINEL).all()) and bool((dW == R.SENTINEL).all())


def test_worst_ratios(capsys):
    """Prints the worst ratio of each output over the tests of this file that ran (nothing to assert beyond them)."""
    with capsys.disabled():
        print('\nencoder tail on the GPU: worst (error - floor) / (UNIT[parts] condition) by output and parts, and K')
        for (n_, p), w in sorted(WORST.items()):
            print(f'  {n_:12s} parts {p} {w:10.3g}   {R.K[n_]}')
    assert all(w <= R.K[n_] for (n_, _), w in WORST.items())
