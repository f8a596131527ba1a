"""CPU checks of tests/gemm_f32_ref.py, the float64 reference of the exact-fp32 entry points (tvae_linear_fwd / _dgrad / _wgrad,
tvae_conv1_fwd / _wgrad): its unfold against torch's convolution, the route of every case through the host queries
(tvae_conv1_f32_route, tvae_linear_f32_route: no device), every route id reached, the budget constants K from plain fp32 torch
arithmetic, and the teeth of the bound (mutations of an fp32 result that it has to reject)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_f32_ref as G

F32 = torch.float32


@pytest.fixture(autouse=True, scope='module')
def one_thread():
    """The summation order of torch's fp32 products follows the thread count: with one thread K is the machine's alone, and a
    mutant that changes no value is bit for bit the clean result."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(threads)


def q(name, *args):
    from tvae import _lib
    return _lib.query(name, *args)


def conv_route(geom, ws, which):
    return q('tvae_conv1_f32_route', *geom, ws, which)


# ---- every case once: tensors, float64 reference, condition quantity, the fp32 CPU result ---------------------------------
def all_cases():
    """(output, case id, tensors, fn) with fn(tensors, dt=, cond=) the case's one expression"""
    for c in G.FWD_CASES:
        yield 'fwd', c['name'], G.fwd_tensors(c), functools.partial(lambda t, c, **kw: G.fwd_ref(c, t, **kw), c=c)
    for c in G.DGRAD_CASES:
        yield 'dgrad', c['name'], G.dgrad_tensors(c), functools.partial(lambda t, c, **kw: G.dgrad_ref(c, t, **kw), c=c)
    for c in G.WGRAD_CASES:
        for acc in (0, 1):
            yield 'wgrad', f"{c['name']}_acc{acc}", G.wgrad_tensors(c), \
                functools.partial(lambda t, c, acc, **kw: G.wgrad_ref(c, t, acc, **kw), c=c, acc=acc)
    for name, geom, act, _ in G.CONV_FWD_CASES:
        yield 'conv_fwd', name, G.conv_fwd_tensors(geom), \
            functools.partial(lambda t, geom, act, **kw: G.conv_fwd_ref(geom, act, t, **kw), geom=geom, act=act)
    for name, geom, _, _ in G.CONV_WGRAD_CASES:
        yield 'conv_wgrad', name, G.conv_wgrad_tensors(geom), \
            functools.partial(lambda t, geom, **kw: G.conv_wgrad_ref(geom, t, **kw), geom=geom)


@functools.cache
def evaluated():
    out = {}
    for output, name, t, fn in all_cases():
        out[output, name] = dict(t=t, fn=fn, ref=fn(t, dt=G.F64, cond=False), cond=fn(t, dt=G.F64, cond=True),
                                 f32=fn(t, dt=F32, cond=False))
    return out


def case(output, name):
    return evaluated()[output, name]


# ---- the unfold references ---------------------------------------------------------------------------------------------
def test_unfold_references_match_torch():
    for B, Cin, n, k, pad, C, R in [(2, 3, 9, 4, 2, 3, 4), (3, 1, 7, 7, 3, 2, 2), (2, 2, 8, 1, 0, 5, 1), (1, 1, 5, 3, 4, 2, 4)]:
        g = G.geom_of(B, Cin, n, k, pad, C, R)
        y, bank, bias = G.rnd(B, Cin, n, n, seed=1).double(), G.rnd(C * R, Cin * k * k, seed=2).double(), G.rnd(C, seed=3).double()
        want = F.conv2d(y, bank.view(C * R, Cin, k, k), None, 1, pad).view(B, C, R, g['P']) + bias.view(1, C, 1, 1)
        got = G.conv_fwd(y, bank, bias, R, k, pad, 0).view(C, B, R, g['P']).permute(1, 0, 2, 3)
        assert (got - want).abs().max() <= 1e-12 * want.abs().max()
        assert torch.equal(G.conv_fwd(y, bank, bias, R, k, pad, 1), F.leaky_relu(G.conv_fwd(y, bank, bias, R, k, pad, 0), G.SLOPE))
        dy = G.rnd(B, C, R, g['Ho'], g['Ho'], seed=4).double()
        want = torch.nn.grad.conv2d_weight(y, (C * R, Cin, k, k), dy.view(B, C * R, g['Ho'], g['Ho']), padding=pad)
        got = G.conv_wgrad(y, dy.permute(1, 0, 2, 3, 4).reshape(C, -1), R, k, pad)
        assert (got.view(C * R, Cin, k, k) - want).abs().max() <= 1e-12 * want.abs().max()
        # the condition quantity is the same expression on absolute values
        assert torch.equal(G.conv_fwd(y, bank, bias, R, k, pad, 2, cond=True), G.conv_fwd(y.abs(), bank.abs(), bias.abs(), R, k, pad, 0))


def test_planted_values_are_where_the_docstring_says():
    assert G.single_positions(400) == [0, 399, 383] and G.single_positions(32) == [0, 31, 15] and G.single_positions(17) == [0, 16, 15]
    assert G.single_positions(16) == [0, 15, 8] and G.single_positions(1) == [0, 0, 0]
    W = G.fwd_tensors(G.FWD_CASES[0])['W']
    assert [(int((W[r] != 0).sum()), int(W[r].nonzero()[0])) for r in range(3)] == [(1, 0), (1, 16), (1, 15)]
    assert 0 < W[3].abs().max() < 2.0 ** -18 < W[4].abs().max()
    aux = G.dgrad_tensors(G.DGRAD_CASES[0])['aux']                     # K = 129 rows, N = 127 columns: column 127 is outside
    assert aux[0, 0] == 0 and not math.copysign(1, aux[0, 0]) < 0 and math.copysign(1, float(aux[0, 31])) < 0 and aux[0, 31] == 0
    assert float(aux[0, 32]) == float(torch.tensor(1e-30)) and int((aux == 0).sum()) == 6
    # a forward case with a residual: the last row's pre-activations lie within rounding of 0, far below their condition quantity
    e = case('fwd', 'glds_vec_pad4_res')
    pre = G.fwd(e['t']['W'], e['t']['X'], e['t']['bias'], None, 0, e['t']['res'], 0)
    assert (pre[-1].abs() <= 4 * G.UNIT * e['cond'][-1]).all() and (pre[-2].abs() > 1e-3).any()


# ---- routes ----------------------------------------------------------------------------------------------------------------
def test_conv_cases_reach_the_routes_they_are_named_for():
    for name, geom, act, route in G.CONV_FWD_CASES:
        assert conv_route(geom, 0, 0) == route, (name, conv_route(geom, 0, 0))
    for name, geom, route, by_ws in G.CONV_WGRAD_CASES:
        g = G.geom_of(*geom)
        assert set(by_ws) == set(G.CONV_WS_KINDS)
        for kind, (slices, ips) in by_ws.items():
            ws = G.conv_ws_floats(kind, g['M'] * g['K'])
            got = tuple(conv_route(geom, ws, w) for w in (1, 2, 3))
            assert got == (route, slices, ips), (name, kind, got)
    # what the names promise beyond the instance, from the kernels' documented formulas
    geoms = {name: geom for name, geom, *_ in G.CONV_FWD_CASES}
    assert G.geom_of(*geoms['img_ragged_tile'])['P'] == 144 and G.geom_of(*geoms['two_exact_tiles'])['P'] == 256
    assert G.geom_of(*geoms['img_vec_three_row_tiles'])['M'] == 384 and G.geom_of(*geoms['generic_m256'])['M'] == 256
    assert all(G.geom_of(*geoms[n])['K'] % 16 for n in ('generic_cin3_ragged_k', 'generic_cin1_ragged_k'))
    assert any(nk == 0 for _, _, nk in G.conv_fwd_tile_ranges(geoms['nk0_tiles']))
    assert any(nk > 0 for _, _, nk in G.conv_fwd_tile_ranges(geoms['nk0_tiles']))
    rng, Kz = G.conv_fwd_tile_ranges(geoms['zero_skip_both_ends']), G.geom_of(*geoms['zero_skip_both_ends'])['K']
    assert any(kb > 0 for kb, _, _ in rng) and any(ks < Kz for _, ks, _ in rng)
    # the XCD id mapping of the weight gradient needs tilesM * slices = 8; the partially resident image of tap tile 1 starts at row 9
    g = G.geom_of(*{name: geom for name, geom, *_ in G.CONV_WGRAD_CASES}['k32_partial_image'])
    rows = min((G.BN - 1) // g['k'] + 2 + g['Ho'] - 1, g['n'] + 2 * g['pad'])
    assert rows < g['n'] + 2 * g['pad'] and G.BN // g['k'] == 9 and g['K'] > G.BN


def test_dense_cases_reach_the_routes_they_are_named_for():
    for op, cases in ((G.OP_FWD, G.FWD_CASES), (G.OP_DGRAD, G.DGRAD_CASES)):
        for c in cases:
            got = tuple(q('tvae_linear_f32_route', *G.dense_route_args(op, c), w) for w in (0, 1, 2))
            assert got == (c['main'], c['ep'], 1), (op, c['name'], got)
    for c in G.WGRAD_CASES:
        per = c['M'] * c['K']
        for kind in G.WS_KINDS:
            for acc in (0, 1):
                got = tuple(q('tvae_linear_f32_route', *G.dense_route_args(G.OP_WGRAD, c, G.ws_floats(kind, per), acc), w)
                            for w in (0, 1, 2))
                want = {'large': c['slices'], 'two': 2, 'one': 1, 'none': 1}[kind]
                assert got == (c['main'], G.EP_SCALAR, want), (c['name'], kind, acc, got)
    # empty outputs launch nothing
    for op, (M, N, K) in ((0, (0, 128, 16)), (0, (128, 0, 16)), (1, (16, 128, 0)), (1, (16, 0, 128)), (2, (0, 64, 128)), (2, (128, 64, 0))):
        assert [q('tvae_linear_f32_route', op, M, N, K, N, N, 63, 0, 1 << 20, w) for w in (0, 1, 2)] == [G.LIN_NONE, 0, 0]


def test_every_route_id_is_reached():
    assert {r for *_, r in G.CONV_FWD_CASES} == {G.FWD_GENERIC, G.FWD_IMG, G.FWD_IMG_VEC, G.FWD_IMG_VEC2}
    assert {r for _, _, r, _ in G.CONV_WGRAD_CASES} == {G.WG_GENERIC, G.WG_K16, G.WG_K32, G.WG_K32_N2}
    dense = [(op, c['main'], c['ep']) for op, cases in ((0, G.FWD_CASES), (1, G.DGRAD_CASES)) for c in cases]
    # each of generic, LDS-DMA + vector epilogue, LDS-DMA + scalar epilogue, for the forward and for the data gradient
    assert set(dense) == {(0, G.LIN_GENERIC, 0), (0, G.LIN_GLDS, 1), (0, G.LIN_GLDS, 0),
                          (1, G.LIN_GENERIC, 0), (1, G.LIN_GLDS2, 1), (1, G.LIN_GLDS2, 0)}
    assert {c['main'] for c in G.WGRAD_CASES} == {G.LIN_GENERIC, G.LIN_V4}
    # (LIN_NONE: the empty shapes of test_dense_cases_reach_the_routes_they_are_named_for, run on the GPU by test_empty_outputs)
    # more than 16 slices (the unrolled loop of splitk_finalize_kernel), by both families
    assert max(c['slices'] for c in G.WGRAD_CASES) > 16
    assert max(by_ws['large'][0] for *_, by_ws in G.CONV_WGRAD_CASES) > 16
    # several images per slice, the direct store, and a slice count that is a multiple of 8 with one row tile (the XCD id mapping)
    res = [v for *_, by_ws in G.CONV_WGRAD_CASES for v in by_ws.values()]
    assert any(ips > 1 and s > 1 for s, ips in res) and any(s == 1 for s, _ in res) and any(s == 8 for s, _ in res)


def test_the_queries_refuse_what_the_entry_points_refuse():
    for geom in [(2, 1, 12, 5, 2, 3, 3), (2, 1, 12, 5, 2, 3, 12), (2, 1, 12, 5, 2, 3, 0), (2, 1, 4, 9, 2, 3, 4), (2, 1, 4, 10, 2, 3, 4)]:
        assert [conv_route(geom, 1 << 20, w) for w in range(4)] == [-1] * 4, geom
    assert conv_route((2, 1, 12, 5, 2, 3, 4), 0, 4) == -1 and conv_route((2, 1, 12, 5, 2, 3, 4), 0, -1) == -1
    assert q('tvae_linear_f32_route', 3, 128, 128, 16, 128, 128, 63, 0, 0, 0) == -1
    assert q('tvae_linear_f32_route', 0, 128, 128, 16, 128, 128, 63, 0, 0, 3) == -1


# ---- the budget constants ----------------------------------------------------------------------------------------------
def test_budget_constants(capsys):
    """K[name] = max(16, 8 x the worst ratio of plain fp32 torch arithmetic against the float64 reference), over every case.
    Printed; gemm_f32_ref.K has to cover it, and not by more than a quarter."""
    worst = {}
    for (output, name), e in evaluated().items():
        r = G.ratio(e['f32'], e['ref'], e['cond'])
        assert math.isfinite(r), (output, name)
        worst[output] = max(worst.get(output, 0.0), r)
    with capsys.disabled():
        print('\n    output       ratio     8 x     K')
        for output, r in worst.items():
            print(f'    {output:<12} {r:6.3f}  {8 * r:6.2f}  {max(16, math.ceil(8 * r)):4d}')
    for output, r in worst.items():
        assert r > 0 and max(16.0, 8 * r) <= G.K[output] <= max(16.0, 8 * r) * 1.25, (output, r, G.K[output])
    assert not G.GPU_SEEN or set(G.GPU_SEEN) == set(G.K)


def test_ratio_helper_is_strict():
    ref, cond = torch.tensor([1.0, 2.0, 0.0], dtype=G.F64), torch.tensor([1.0, 2.0, 0.0], dtype=G.F64)
    assert G.ratio(ref.float(), ref, cond) == 0.0
    assert G.ratio(torch.tensor([1.0, 2.0, 1e-30]), ref, cond) == math.inf                  # exact where the condition is zero
    assert G.ratio(torch.tensor([1.0, float('nan'), 0.0]), ref, cond) == math.inf            # an element nobody wrote
    assert G.ratio(torch.tensor([1.0, 2.0, -0.0]), ref, cond) == 0.0
    assert abs(G.ratio(torch.tensor([1.0 + 2.0 ** -20, 2.0, 0.0]), ref, cond) - 16.0) < 1e-6
    assert abs(G.ratio(torch.tensor([1.0 + 2.0 ** -20, 2.0, 0.0]), ref, cond, 16.0) - 1.0) < 1e-6


# ---- the bound has teeth --------------------------------------------------------------------------------------------------
def _mutants(output, name, e):
    """(defect, fp32 result with the defect) for one case"""
    t, fn = e['t'], e['fn']

    def run(**changed):
        return fn({**t, **changed}, dt=F32, cond=False)

    def edit(key, f):
        x = t[key].clone()
        f(x)
        return {key: x}
    if output == 'fwd':
        c = next(c for c in G.FWD_CASES if c['name'] == name)
        yield 'last reduction step dropped', run(**edit('W', lambda W: W[:, -1].zero_()))
        if c['pa']:
            yield 'pad column read as data', run(**edit('X', lambda X: X[:, -1].fill_(G.PAD_IN)))
    elif output == 'dgrad':
        c = next(c for c in G.DGRAD_CASES if c['name'] == name)
        yield 'last reduction step dropped', run(**edit('W', lambda W: W[-1].zero_()))
        if c['pa']:
            yield 'pad column read as data', run(**edit('dpre', lambda d: d[:, -1].fill_(G.PAD_IN)))
        if c['act'] == 1 and c['aux']:
            yield 'aux == 0 treated as positive', run(**edit('aux', lambda a: a.masked_fill_(a == 0, 1.0)))
    elif output == 'wgrad':
        c = next(c for c in G.WGRAD_CASES if name.startswith(c['name']))
        yield 'last reduction step dropped', run(**edit('dpre', lambda d: d[:, -1].zero_()))
        if c['pa'] or c['pb']:
            pad = lambda x: torch.cat([x, torch.full((x.shape[0], 1), 1e15)], 1)        # (PAD_IN x PAD_IN overflows: 1e15 here)
            yield 'pad column read as data', run(dpre=pad(t['dpre']), X=pad(t['X']))
    elif output == 'conv_fwd':
        geom = next(g for n, g, *_ in G.CONV_FWD_CASES if n == name)
        act = next(a for n, _, a, _ in G.CONV_FWD_CASES if n == name)
        g = G.geom_of(*geom)
        yield 'last reduction step dropped', run(**edit('bank', lambda b: b[:, -1].zero_()))
        yield 'one tap row skipped', run(**edit('bank', lambda b: b.view(g['M'], g['Cin'], g['k'], g['k'])[:, 0, g['k'] // 2].zero_()))
        pre = G.conv_fwd(t['y'], t['bank'], None, g['R'], g['k'], g['pad'], 0, dt=F32).view(g['C'], g['B'], g['R'], g['P'])
        bias_m = t['bias'][torch.arange(g['M']) % g['C']].view(g['C'], 1, g['R'], 1)
        yield 'bias indexed m instead of m >> log2 R', G.act_apply(pre + bias_m, act).reshape(g['C'], -1)
    else:
        geom = next(g for n, g, *_ in G.CONV_WGRAD_CASES if n == name)
        g = G.geom_of(*geom)
        yield 'last reduction step dropped', run(**edit('dpre', lambda d: d.view(g['C'], g['B'], g['R'], g['P'])[:, -1, :, -1].zero_()))
        yield 'image of the last slice dropped', run(**edit('y', lambda y: y[-1].zero_()))
        skipped = e['f32'].clone()
        skipped.view(g['M'], g['Cin'], g['k'], g['k'])[:, 0, g['k'] // 2].zero_()
        yield 'one tap row skipped', skipped


def test_the_bound_rejects_every_mutation():
    """Each defect is applied to the fp32 CPU result of every case it applies to; wherever it changes a value at all, the bound --
    at the K of the module -- has to reject the result.  The clean fp32 result passes (test_budget_constants)."""
    seen, missed = {}, []
    for (output, name), e in evaluated().items():
        assert G.ratio(e['f32'], e['ref'], e['cond'], G.K[output]) <= 1.0, (output, name)
        for defect, mut in _mutants(output, name, e):
            if torch.equal(mut, e['f32']):
                continue
            seen[defect] = seen.get(defect, 0) + 1
            if not G.ratio(mut, e['ref'], e['cond'], G.K[output]) > 1.0:
                missed.append((output, name, defect))
    assert not missed, missed
    assert set(seen) == {'last reduction step dropped', 'one tap row skipped', 'aux == 0 treated as positive',
                         'image of the last slice dropped', 'pad column read as data', 'bias indexed m instead of m >> log2 R'}
    assert min(seen.values()) >= 3, seen
