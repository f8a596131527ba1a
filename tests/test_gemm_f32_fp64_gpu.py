"""The exact-fp32 entry points -- tvae_linear_fwd / _dgrad / _wgrad and tvae_conv1_fwd / _wgrad -- against tests/gemm_f32_ref.py in
float64, one case for every kernel instance, epilogue, split and slicing they can take (case lists and planted values:
gemm_f32_ref.py; tests/test_gemm_f32_ref_cpu.py proves on the host that the lists reach every route id of tvae_conv1_f32_route /
tvae_linear_f32_route, and every test here asserts the route of ITS call with the same queries before it launches).

EVERY element of every output against K 2^-24 (condition quantity) + TINY, exactly where the condition quantity is zero (K comes
from CPU arithmetic, never from these kernels).  Outputs start as NaN, so an element nobody writes fails; strided inputs carry
1e30 in their pad columns, strided outputs a sentinel that has to come back untouched; workspaces start as NaN.  Pointers are
misaligned by taking a view one float into a larger buffer.  Refusals are exact: an error, and every output still holds its
prefill.  Every call runs between guard bands, twice (replay): two runs of one call agree bit for bit.

Worst ratio seen on an MI355X, by output: gemm_f32_ref.GPU_SEEN; test_worst_ratios prints this run's."""
import functools
import math

import pytest
import torch

import gemm_f32_ref as G
import guardband

pytestmark = pytest.mark.gpu
WORST = {}
SLOPE = 0.01
NAN = float('nan')


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in test_hip_primitives.py: every C-ABI call on relocated tensors between guard bands, twice from the same inputs."""
    with guardband.GuardedCalls(replay=True):
        yield


def dev():
    return torch.device('cuda:0')


def call(*a, **kw):
    from tvae._lib import call as c
    return c(*a, **kw)


def query(*a):
    from tvae._lib import query as q
    return q(*a)


def place(t, mis=False):
    """t on the device, 16-byte aligned -- or, mis, as a view one float into a larger buffer (address = 4 mod 16)"""
    if t is None:
        return None
    t = t.contiguous()
    if not mis:
        t = t.to(dev())
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(t.numel() + 4, device=dev())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def align_mask(*tensors):
    return sum(1 << i for i, t in enumerate(tensors) if t is None or t.data_ptr() % 16 == 0)


def check(name, got, ref, cond, what):
    r = G.ratio(got.cpu(), ref, cond)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f'{name} {what}: ratio {r:.3f} of K = {G.K[name]}')
    assert math.isfinite(r) and r <= G.K[name], (name, what, r, G.K[name])


def pads_untouched(T, N):
    assert bool((T[:, N:] == G.SENTINEL).all()), 'pad columns of a strided output were written'


# ---- references: once per case, shared by the tests that need them, never changed ------------------------------------------
@functools.cache
def conv_fwd_case(name):
    _, geom, act, route = next(c for c in G.CONV_FWD_CASES if c[0] == name)
    t = G.conv_fwd_tensors(geom)
    return geom, act, route, t, G.conv_fwd_ref(geom, act, t), G.conv_fwd_ref(geom, act, t, cond=True)


@functools.cache
def conv_wgrad_case(name):
    _, geom, route, by_ws = next(c for c in G.CONV_WGRAD_CASES if c[0] == name)
    t = G.conv_wgrad_tensors(geom)
    return geom, route, by_ws, t, G.conv_wgrad_ref(geom, t), G.conv_wgrad_ref(geom, t, cond=True)


@functools.cache
def wgrad_case(name):
    c = next(c for c in G.WGRAD_CASES if c['name'] == name)
    t = G.wgrad_tensors(c)
    return c, t, {acc: (G.wgrad_ref(c, t, acc), G.wgrad_ref(c, t, acc, cond=True)) for acc in (0, 1)}


# ---- lifting convolution ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c[0] for c in G.CONV_FWD_CASES])
def test_conv1_fwd(name):
    geom, act, route, t, ref, cond = conv_fwd_case(name)
    g = G.geom_of(*geom)
    assert query('tvae_conv1_f32_route', *geom, 0, 0) == route
    out = torch.full((g['C'], g['B'] * g['R'] * g['P']), NAN, device=dev())
    call('tvae_conv1_fwd', place(t['y']), place(t['bank']), place(t['bias']), out, *geom, act, SLOPE)
    check('conv_fwd', out, ref, cond, f'{name} route {route}')
    # where every tap meets zero padding the output is act(bias), bit for bit (tiles with an empty k range among them)
    only_pad = G.conv_fwd(t['y'], t['bank'], None, g['R'], g['k'], g['pad'], 0, cond=True) == 0
    if name in ('pad_only_tiles_k1', 'nk0_tiles'):
        assert act in (0, 1) and int(only_pad.sum()) > 128 * g['M']
    if act in (0, 1):
        want = G.act_apply(t['bias'], act)[:, None].expand(g['C'], g['B'] * g['R'] * g['P'])
        # (rows with ONE bank entry meet padding there too; the whole tile has to, so the plain rows decide)
        assert torch.equal(out.cpu()[only_pad], want[only_pad])


@pytest.mark.parametrize('kind', G.CONV_WS_KINDS)
@pytest.mark.parametrize('name', [c[0] for c in G.CONV_WGRAD_CASES])
def test_conv1_wgrad(name, kind):
    geom, route, by_ws, t, ref, cond = conv_wgrad_case(name)
    g = G.geom_of(*geom)
    nws = G.conv_ws_floats(kind, g['M'] * g['K'])
    got_route = tuple(query('tvae_conv1_f32_route', *geom, nws, w) for w in (1, 2, 3))
    assert got_route == (route,) + by_ws[kind]
    dbank = torch.full((g['M'], g['K']), NAN, device=dev())
    ws = torch.full((nws,), NAN, device=dev()) if nws else None
    call('tvae_conv1_wgrad', place(t['y']), place(t['dpre']), dbank, ws, nws, *geom)
    check('conv_wgrad', dbank, ref, cond, f'{name} ws {kind}: route {got_route}')


def test_conv1_refusals_write_nothing():
    """R = 3 and Ho <= 0: both entry points return an error before any launch; outputs and workspace keep their prefill."""
    from tvae._lib import TvaeHipError
    for geom in ((2, 1, 12, 5, 2, 3, 3), (2, 1, 4, 9, 2, 3, 4), (2, 1, 4, 10, 2, 3, 4)):
        B, Cin, n, k, pad, C, R = geom
        assert [query('tvae_conv1_f32_route', *geom, 1 << 16, w) for w in range(4)] == [-1] * 4
        P = max(n + 2 * pad - k + 1, 1) ** 2
        y, bank, bias = torch.rand(B, Cin, n, n, device=dev()), torch.rand(C * R, Cin * k * k, device=dev()), torch.rand(C, device=dev())
        out, dbank = torch.full((C, B * R * P), 7.0, device=dev()), torch.full((C * R, Cin * k * k), 7.0, device=dev())
        ws = torch.full((1 << 16,), 7.0, device=dev())
        with pytest.raises(TvaeHipError):
            call('tvae_conv1_fwd', y, bank, bias, out, *geom, 1, SLOPE)
        with pytest.raises(TvaeHipError):
            call('tvae_conv1_wgrad', y, out, dbank, ws, ws.numel(), *geom)
        torch.cuda.synchronize()
        for x in (out, dbank, ws):
            assert bool((x == 7.0).all())


# ---- dense forward and data gradient -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in G.FWD_CASES])
def test_linear_fwd(name):
    c = next(c for c in G.FWD_CASES if c['name'] == name)
    M, N, K_, ldx, ldy, mis = c['M'], c['N'], c['K'], c['N'] + c['pa'], c['N'] + c['pb'], c['mis']
    t = G.fwd_tensors(c)
    W, X, b = place(t['W'], mis == 'W'), place(G.strided(t['X'], ldx), mis == 'X'), place(t['bias'], mis == 'bias')
    gb = place(t['gbias'], mis == 'gbias')
    res = place(None if t['res'] is None else G.strided(t['res'], ldy), mis == 'res')
    Y = place(G.blank(M, N, ldy), mis == 'Y')
    mask = align_mask(W, X, b, gb, res, Y)
    args = G.dense_route_args(G.OP_FWD, c)
    assert mask == args[6]                                     # (an absent pointer counts as aligned)
    route = tuple(query('tvae_linear_f32_route', *args[:6], mask, *args[7:], w) for w in (0, 1, 2))
    assert route == (c['main'], c['ep'], 1), route
    call('tvae_linear_fwd', W, X, b, gb, c['group'], res, Y, M, N, K_, ldx, ldy, c['act'], SLOPE)
    check('fwd', Y[:, :N], G.fwd_ref(c, t), G.fwd_ref(c, t, cond=True), f'{name} route {route}')
    pads_untouched(Y, N)


@pytest.mark.parametrize('name', [c['name'] for c in G.DGRAD_CASES])
def test_linear_dgrad(name):
    c = next(c for c in G.DGRAD_CASES if c['name'] == name)
    M, N, K_, ldd, ldx, mis = c['M'], c['N'], c['K'], c['N'] + c['pa'], c['N'] + c['pb'], c['mis']
    t = G.dgrad_tensors(c)
    W, d = place(t['W'], mis == 'W'), place(G.strided(t['dpre'], ldd), mis == 'dpre')
    add = place(None if t['add'] is None else G.strided(t['add'], ldx), mis == 'add')
    aux = place(None if t['aux'] is None else G.strided(t['aux'], ldx), mis == 'aux')      # (given with mask 0 too: then unread)
    dX = place(G.blank(K_, N, ldx), mis == 'dX')
    args = G.dense_route_args(G.OP_DGRAD, c)
    route = tuple(query('tvae_linear_f32_route', *args[:6], align_mask(W, d, add, aux, dX), *args[7:], w) for w in (0, 1, 2))
    assert route == (c['main'], c['ep'], 1), route
    call('tvae_linear_dgrad', W, d, add, aux, dX, M, N, K_, ldd, ldx, c['act'], SLOPE)
    check('dgrad', dX[:, :N], G.dgrad_ref(c, t), G.dgrad_ref(c, t, cond=True), f'{name} route {route}')
    pads_untouched(dX, N)


# ---- dense weight gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('kind', G.WS_KINDS)
@pytest.mark.parametrize('name', [c['name'] for c in G.WGRAD_CASES])
def test_linear_wgrad(name, kind, acc):
    """Results under different workspace sizes are each held to the bound, not to each other: the slice count follows the
    workspace.  'one' (a single slab) and 'none' run without split-K -- with accumulate, straight into dW."""
    c, t, refs = wgrad_case(name)
    M, N, K_, ldd, ldx, mis = c['M'], c['N'], c['K'], c['N'] + c['pa'], c['N'] + c['pb'], c.get('mis')
    nws = G.ws_floats(kind, M * K_)
    d, X = place(G.strided(t['dpre'], ldd), mis == 'dpre'), place(G.strided(t['X'], ldx), mis == 'X')
    dW = place(t['init'].clone() if acc else torch.full((M, K_), NAN))
    ws = torch.full((nws,), NAN, device=dev()) if nws else None
    args = G.dense_route_args(G.OP_WGRAD, c, nws, acc)
    route = tuple(query('tvae_linear_f32_route', *args[:6], align_mask(d, X, dW, ws), *args[7:], w) for w in (0, 1, 2))
    assert route == (c['main'], G.EP_SCALAR, {'large': c['slices'], 'two': 2, 'one': 1, 'none': 1}[kind]), route
    call('tvae_linear_wgrad', d, X, dW, ws, nws, M, N, K_, ldd, ldx, acc)
    check('wgrad', dW, *refs[acc], f'{name} ws {kind} acc {acc}: route {route}')


def test_empty_outputs_succeed_and_write_nothing():
    """M = 0 and N = 0 (the data gradient: K = 0, the weight gradient: M = 0 and K = 0): success, and nothing is written."""
    seven = lambda *s: torch.full(s, 7.0, device=dev())
    e = lambda *s: torch.empty(s, device=dev())
    r = lambda *s: torch.rand(s, device=dev())
    assert query('tvae_linear_f32_route', 0, 0, 128, 16, 128, 128, 63, 0, 0, 0) == G.LIN_NONE
    call('tvae_linear_fwd', e(0, 16), r(16, 128), e(0), None, 0, None, e(0, 128), 0, 128, 16, 128, 128, 1, SLOPE)
    Y = seven(128, 4)
    call('tvae_linear_fwd', r(128, 16), seven(16, 4), r(128), None, 0, None, Y, 128, 0, 16, 4, 4, 1, SLOPE)
    call('tvae_linear_fwd', e(0, 17), r(17, 100), e(0), None, 0, None, e(0, 100), 0, 100, 17, 100, 100, 1, SLOPE)
    dX = seven(128, 4)
    call('tvae_linear_dgrad', r(16, 128), seven(16, 4), None, None, dX, 16, 0, 128, 4, 4, 0, SLOPE)
    call('tvae_linear_dgrad', e(16, 0), r(16, 128), None, None, e(0, 128), 16, 128, 0, 128, 128, 0, SLOPE)
    ws = seven(1 << 16)
    call('tvae_linear_wgrad', e(0, 64), r(128, 64), e(0, 128), ws, ws.numel(), 0, 64, 128, 64, 64, 0)
    call('tvae_linear_wgrad', r(128, 64), e(0, 64), e(128, 0), ws, ws.numel(), 128, 64, 0, 64, 64, 1)
    torch.cuda.synchronize()
    for x in (Y, dX, ws):
        assert bool((x == 7.0).all())


def test_worst_ratios(capsys):
    """Prints the worst ratio of each output over the tests of this file that ran (nothing to assert beyond them)."""
    with capsys.disabled():
        print('\nexact-fp32 GEMM and lifting-conv routes on the GPU: worst |error| / (2^-24 condition) by output, and K')
        for n_, w in sorted(WORST.items()):
            print(f'  {n_:12s} {w:10.3g}   {G.K[n_]}')
    assert all(w <= G.K[n_] for n_, w in WORST.items())
