"""hipGraph replay against eager execution, BIT FOR BIT, on every route a driver can capture.

The drivers capture forward + backward into a hipGraph wherever tvae.driver.graph_supported() allows it, so the replay -- not
the eager step every other test of the suite runs -- is what trains.  Each case of step_cases.GRAPH_CASES runs a trajectory
of three optimizer steps twice from the same seeded state, eagerly and through tvae.graph.GraphedStep: gradients, ELBO terms
and the optimizer state must be the same bits, and the two runs must have taken the same routes of tvae/ops.py.  The last
test closes the coverage: every route name ops.py can record was replayed by some case, or is listed with its reason in
step_cases.GRAPH_EXCLUDED_ROUTES.

Every comparison here is torch.equal.  Nothing runs under guardband.GuardedCalls (it relocates tensors, which a captured graph
cannot follow) and ops.KERNEL_EVENTS stays off (events are recorded host-side)."""
import contextlib

import numpy as np
import pytest
import torch

from step_cases import (GRAPH_ARITHMETIC_CASES, GRAPH_ARITHMETIC_MODES, GRAPH_CASES, GRAPH_EXCLUDED_ROUTES, OOB_CONFIGS,
                        cin3_direct_encoder, dev, fresh, golden_step, heads103_encoder, noted_routes)

pytestmark = pytest.mark.gpu
STEPS = 3
LR = 1e-3
REPLAYED = set()          # union of the route sets of every case that was captured and replayed in this session
REPLAYED_BY_CASE = {}


def _build(case, batch=None):
    """Freshly seeded (gen, enc, x, B, image shape, first minibatch and noise or None) of one GRAPH_CASES row: the same
    bits on every call."""
    import src.models as M
    c = GRAPH_CASES[case]
    first = None
    if 'cfg' in c:
        n, zd, R, B, C, hid, k, pad, four = OOB_CONFIGS[c['cfg']]
        B = batch or c.get('B', B)
        gen, enc, x, _, _ = fresh(n, zd, R, B, C, hid, k, pad, four, **c.get('kw', {}))
        shape = (1, n, n)
    elif 'golden' in c:
        assert batch is None
        fx, enc, gen, x, y, noise = golden_step(c['golden'])
        B, shape, first = y.shape[0], tuple(y.shape[1:]), (y, noise)
    else:
        assert batch is None
        from tvae import tables
        enc, y, zd, R = cin3_direct_encoder() if c['encoder'] == 'cin3_direct' else heads103_encoder(c['encoder'])
        B, shape = y.shape[0], tuple(y.shape[1:])
        gen = M.SpatialGenerator(zd, 32, n_out=shape[0], num_layers=2).to(dev())      # a small plain decoder behind it
        x = torch.from_numpy(tables.image_coords(shape[-1])).to(dev())
    return gen, enc, x, B, shape, first


def _data(case, enc, B, shape, first, steps):
    """A different minibatch and a different noise triple for every step (the fixture's own pair first, where there is one)."""
    from tvae import step
    g = torch.Generator(device=dev()).manual_seed(11)
    unit = GRAPH_CASES[case]['lik'] in ('bce', 'bce3')
    ys, noises = [], []
    for _ in range(steps):
        y = torch.rand((B,) + shape, device=dev(), generator=g)
        ys.append(y if unit else (y - 0.5) * 4.0)
        noises.append(step.draw_noise(B, enc.groupconv * enc.output_size() ** 2, enc.latent_dim, dev(), generator=g))
    if first is not None:
        ys[0], noises[0] = first
    return ys, noises


@contextlib.contextmanager
def _setting(case, mode):
    """Arithmetic mode and routing switches of a case, around BOTH of its runs."""
    from tvae import _lib, ops
    old = ops.CONV_DFT
    if not GRAPH_CASES[case].get('dft', True):
        ops.CONV_DFT = False
    try:
        with _lib.arithmetic(mode):
            yield
    finally:
        ops.CONV_DFT = old


@contextlib.contextmanager
def _routes(into):
    from tvae import ops
    assert ops.PATH_LOG is None and ops.KERNEL_EVENTS is None
    ops.PATH_LOG = set()
    try:
        yield
        into |= ops.PATH_LOG
    finally:
        ops.PATH_LOG = None


def _terms(e, lp, kl):
    return torch.stack([e.detach().double(), lp.detach().double(), kl.detach().double()])


def _eager(case, batch=None, steps=STEPS):
    """The eager trajectory: per step (flat_g, terms) after the backward, the final (flat_p, flat_m, flat_v), the routes taken
    and the data it ran on."""
    from tvae import optim, step
    gen, enc, x, B, shape, first = _build(case, batch)
    ys, noises = _data(case, enc, B, shape, first, steps)
    opt = optim.FlatAdam(list(gen.parameters()) + list(enc.parameters()), lr=LR)
    lik, per_step, routes = GRAPH_CASES[case]['lik'], [], set()
    with _routes(routes):
        for y, nz in zip(ys, noises):
            e, lp, kl = step.elbo_terms(x, y, gen, enc, lik, nz)
            step.backward_neg_elbo(e)
            per_step.append((opt.flat_g.clone(), _terms(e, lp, kl)))
            opt.step()
            opt.zero_grad()
    # the trajectory is worth comparing with: finite, non-zero gradients that differ from step to step
    for i, (g_i, t_i) in enumerate(per_step):
        assert bool(torch.isfinite(g_i).all()) and bool(torch.isfinite(t_i).all()) and float(g_i.abs().max()) > 0, (case, i)
        assert i == 0 or not torch.equal(g_i, per_step[i - 1][0]), (case, i)
    return dict(steps=per_step, final=(opt.flat_p.clone(), opt.flat_m.clone(), opt.flat_v.clone()), routes=routes, ys=ys,
                noises=noises, B=B)


class _Graphed:
    """A freshly seeded model and optimizer behind a GraphedStep; check(i, eager) replays step i and compares."""

    def __init__(self, case, batch=None):
        from tvae import graph, optim
        self.gen, self.enc, self.x, B, shape, _ = _build(case, batch)
        self.opt = optim.FlatAdam(list(self.gen.parameters()) + list(self.enc.parameters()), lr=LR)
        self.routes = set()
        with _routes(self.routes):                      # the two warm-up passes and the capture
            self.gs = graph.GraphedStep(self.x, self.gen, self.enc, self.opt, GRAPH_CASES[case]['lik'], B, shape, dev())

    def check(self, i, eager):
        terms = self.gs.run(eager['ys'][i], eager['noises'][i])
        want_g, want_terms = eager['steps'][i]
        assert torch.equal(self.opt.flat_g.view(torch.int32), want_g.view(torch.int32)), ('flat_g', i)
        assert torch.equal(terms, want_terms), ('terms', i, terms, want_terms)
        self.opt.step()
        self.opt.zero_grad()

    def check_final(self, eager):
        for got, want, nm in zip((self.opt.flat_p, self.opt.flat_m, self.opt.flat_v), eager['final'], 'pmv'):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), 'flat_' + nm

    def close(self):
        self.gs.close()


def _case_params():
    out = [pytest.param(c, id=c) for c in GRAPH_CASES]
    out += [pytest.param(f'{c}@{m}', id=f'{c}@{m}') for c in GRAPH_ARITHMETIC_CASES for m in GRAPH_ARITHMETIC_MODES]
    return out


@pytest.mark.parametrize('case', _case_params())
def test_replay_is_bitwise_eager(case):
    """Three optimizer steps (a different minibatch and noise triple each, FlatAdam lr = 1e-3), eagerly and as replays of
    the captured graph, from the same seeded state: flat_g and the three ELBO terms after every backward, flat_p / flat_m /
    flat_v at the end -- the same bits.  The warm-up passes and the capture took the routes the eager run took."""
    name, _, mode = case.partition('@')
    with _setting(name, mode or 'h3'):
        eager = _eager(name)
        g = _Graphed(name)
        try:
            assert g.routes == eager['routes'], (sorted(g.routes - eager['routes']), sorted(eager['routes'] - g.routes))
            for i in range(STEPS):
                g.check(i, eager)
            g.check_final(eager)
        finally:
            g.close()
    REPLAYED.update(g.routes)
    REPLAYED_BY_CASE[case] = sorted(g.routes)
    print('\nroutes[%s] = %s' % (case, ' '.join(sorted(g.routes))))


def test_replay_survives_eager_work_between_replays():
    """What every epoch's test pass does to an open graph: between two replays the evaluation loop, an eager training step and
    get_latent run on FOUR times the captured batch and outgrow the named scratch buffers the graph holds raw pointers
    into.  The outgrown blocks must stay alive for the graph (ops._PINNED under its token, non-empty), the later replays
    must still be the eager trajectory bit for bit, and close() must release the token."""
    from tvae import latent, ops, step
    case, B = 'S28', 8
    n, zd, R = OOB_CONFIGS[case][:3]
    saved = dict(ops._WS)
    ops._WS.clear()          # buffers of the captured size, whatever larger problem ran earlier in this process
    g = None
    try:
        with _setting(case, 'h3'):
            eager = _eager(case, batch=B)
            g = _Graphed(case, batch=B)
            g.check(0, eager)
            gen, enc, x, opt = g.gen, g.enc, g.x, g.opt
            gb = torch.Generator(device=dev()).manual_seed(12)
            big = torch.randn(4 * B, 1, n, n, device=dev(), generator=gb)
            step.eval_model([(big,)], x, gen, enc, 'attention', 'attention+offsets', 0, dev(), np.pi, R, n, likelihood='gauss')
            gen.train()
            enc.train()
            e, _, _ = step.elbo_terms(x, big, gen, enc, 'gauss')
            step.backward_neg_elbo(e)
            opt.flat_g.zero_()                          # gradients discarded, as GraphedStep.__init__ leaves the buffer
            latent.get_latent(x, big, enc, 'attention', 'attention+offsets', dev(), n)
            assert ops._PINNED.get(g.gs._pin), 'the eager work did not outgrow any buffer the graph points into'
            g.check(1, eager)
            g.check(2, eager)
            g.check_final(eager)
            tok = g.gs._pin
            g.close()
            assert tok not in ops._PINNED
    finally:
        if g is not None:
            g.close()
        ops._WS.clear()
        ops._WS.update(saved)


def test_two_graphs_in_one_process():
    """Two open graphs of the same model family at different batches share every named scratch buffer and the workspace:
    replayed alternately, each follows its own eager trajectory bit for bit, and closing the first leaves the second intact."""
    case = 'S28'
    a = b = None
    with _setting(case, 'h3'):
        try:
            eager_a = _eager(case, batch=8)
            a = _Graphed(case, batch=8)
            a.check(0, eager_a)
            eager_b = _eager(case, batch=16)
            b = _Graphed(case, batch=16)
            a.check(1, eager_a)
            b.check(0, eager_b)
            a.check(2, eager_a)
            b.check(1, eager_b)
            a.check_final(eager_a)
            a.close()
            b.check(2, eager_b)
            b.check_final(eager_b)
        finally:
            for g in (a, b):
                if g is not None:
                    g.close()


@pytest.mark.parametrize('case', ['S28F', 'galaxy'])
def test_train_epoch_with_graph_equals_eager_epoch(case):
    """step.train_epoch over three full minibatches and a ragged tail: replays for the full ones and the eager step for the tail,
    against the all-eager epoch -- the same returned means and the same parameters."""
    from tvae import graph, optim, step
    lik = GRAPH_CASES[case]['lik']
    with _setting(case, 'h3'):
        out = []
        for graphed in (True, False):
            gen, enc, x, B, shape, first = _build(case)
            ys, noises = _data(case, enc, B, shape, first, 4)
            tail = max(B - 1, 1)
            data = torch.cat(ys[:3] + [ys[3][:tail]])
            nz_all = noises[:3] + [tuple(t[:tail] for t in noises[3])]
            it = [(data[i:i + B],) for i in range(0, data.shape[0], B)]
            params = list(gen.parameters()) + list(enc.parameters())
            opt = optim.FlatAdam(params, lr=LR)
            gs = graph.GraphedStep(x, gen, enc, opt, lik, B, shape, dev()) if graphed else None
            try:
                r = step.train_epoch(it, x, gen, enc, opt, 'attention', 'attention+offsets', 0, 1, data.shape[0], dev(), params,
                                     np.pi, enc.groupconv, shape[-1], likelihood=lik, progress=False, noise_iter=iter(nz_all),
                                     graphed=gs)
            finally:
                if gs is not None:
                    gs.close()
            out.append((r, opt.flat_p.clone()))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))


def test_every_capturable_route_was_replayed(request):
    """Keeps the coverage closed: when this whole file has run in the session, every route name tvae/ops.py can record
    (`_note(...)`) was taken by a case that was captured, replayed and found bitwise equal to eager -- or it is listed, with
    its reason, among the routes no captured step can take.  An excluded name that was replayed after all fails too."""
    # (request.session.items holds what is left after a -k / -m / node-id selection)
    ran = {it.name for it in request.session.items if it.path == request.node.path}
    need = {'test_replay_is_bitwise_eager[%s]' % p.id for p in _case_params()}
    need |= {'test_train_epoch_with_graph_equals_eager_epoch[%s]' % c for c in ('S28F', 'galaxy')}
    need |= {k_ for k_, v_ in globals().items() if k_.startswith('test_') and callable(v_)} - \
        {'test_replay_is_bitwise_eager', 'test_train_epoch_with_graph_equals_eager_epoch'}
    if not need <= ran:
        pytest.skip('only meaningful when the whole file runs (a -k / -m / node-id selection left part of it out)')
    routes = noted_routes()
    assert all(isinstance(r, str) and r for r in GRAPH_EXCLUDED_ROUTES.values())
    stale = sorted(set(GRAPH_EXCLUDED_ROUTES) & REPLAYED)
    assert not stale, f'excluded routes that a captured step did take: {stale}'
    missing = sorted(routes - set(GRAPH_EXCLUDED_ROUTES) - REPLAYED)
    assert not missing, f'routes of tvae/ops.py that no replayed case took: {missing}'
    assert REPLAYED <= routes, sorted(REPLAYED - routes)
