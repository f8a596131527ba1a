"""The overlap rule of the four entry points of libtvae_cluster.so that had no test of it: tvae_pose_refine,
tvae_pose_classify, tvae_pose_posterior and tvae_class_average_weighted reject a call in which an output shares a byte with
an input, on the host and before any launch, and write nothing (tests/test_polish_gpu.py and tests/test_eigen_gpu.py test
tvae_pose_moments, tvae_pose_polish_step, tvae_class_project and tvae_class_backproject).  Every call here pairs an OUTPUT
with an INPUT: no two outputs overlap anywhere, so no call is one that an entry point might accept.  One valid call per
entry point at the same shape succeeds under the guard bands."""
import numpy as np
import pytest
import torch

import guardband

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SENT_F = -12345.5
SENT_I = -7777777
N, C, n, K, A, S, M, P = 3, 1, 8, 2, 1, 1, 2, 2
CAND = (2 * A + 1) * (2 * S + 1) ** 2           # candidate poses of an (image, slot)
PLANE = C * n * n


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


def _sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENT_I if dtype == torch.int32 else SENT_F, dtype=dtype, device=DEV)


def _inputs():
    g = torch.Generator().manual_seed(5)
    return dict(Y=torch.randn(N, C, n, n, generator=g).to(DEV), theta=torch.zeros(N, device=DEV), dx=torch.zeros(N, 2, device=DEV),
                cls=torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV), ref=torch.randn(K, C, n, n, generator=g).to(DEV),
                cand=torch.tensor([[0, 1], [1, 0], [0, -1]], dtype=torch.int32, device=DEV))


def _overlapping(in_words, out_words, shared):
    """One sentinel-filled buffer, an input of in_words at its start and an output of out_words that begins `shared` words before
    the input ends -> (buffer, input view, output view)."""
    assert 0 < shared <= min(in_words, out_words)
    flat = _sent(in_words + out_words - shared)
    return flat, flat[:in_words], flat[in_words - shared:in_words - shared + out_words]


def _rejected(name, *args):
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    with pytest.raises(TvaeHipError, match=name + ' failed'):
        with guardband.GuardedCalls():                       # a rejected call must leave every tensor as it was
            CL.call(name, *args)


def _accepted(name, *args):
    from tvae import _cluster_lib as CL
    with guardband.GuardedCalls():
        CL.call(name, *args)
    torch.cuda.synchronize()


def _all_sentinels(*tensors):
    for i, t in enumerate(tensors):
        assert bool((t == (SENT_I if t.dtype == torch.int32 else SENT_F)).all()), i


def test_pose_refine():
    i = _inputs()
    wsf = N * (2 * CAND + 1)
    o = dict(theta_out=_sent(N), dx_out=_sent(N, 2), score=_sent(N, 2), best=_sent(N, 3, dtype=torch.int32), num=_sent(N, CAND),
             pp=_sent(N, CAND), yy=_sent(N), ws=_sent(wsf))
    tail = (wsf, N, C, n, K, A, S, 1.0, 0.1, 0.0, 0.0)
    flat, dx, theta_out = _overlapping(2 * N, N, 2)           # theta_out begins inside dx
    _rejected('tvae_pose_refine', i['Y'], i['theta'], dx.view(N, 2), i['cls'], i['ref'], theta_out, o['dx_out'], o['score'], o['best'],
              None, None, None, o['ws'], *tail)
    _all_sentinels(flat, *o.values())
    flat, Y, num = _overlapping(N * PLANE, N * CAND, 2)       # the optional table num begins inside Y
    _rejected('tvae_pose_refine', Y.view(N, C, n, n), i['theta'], i['dx'], i['cls'], i['ref'], o['theta_out'], o['dx_out'], o['score'],
              o['best'], num.view(N, CAND), o['pp'], o['yy'], o['ws'], *tail)
    _all_sentinels(flat, *o.values())
    _accepted('tvae_pose_refine', i['Y'], i['theta'], i['dx'], i['cls'], i['ref'], *o.values(), *tail)
    assert bool(torch.isfinite(o['score']).all()) and bool((o['yy'] > 0).all())


def test_pose_classify_and_posterior():
    i = _inputs()
    table = M * CAND
    wsf = N * (2 * table + 1)
    o = dict(cls_out=_sent(N, dtype=torch.int32), best=_sent(N, 4, dtype=torch.int32), theta_out=_sent(N), dx_out=_sent(N, 2),
             score=_sent(N, M, 2), num=_sent(N, table), pp=_sent(N, table), yy=_sent(N), ws=_sent(wsf))
    tail = (wsf, N, C, n, K, M, A, S, 1.0, 0.1, 0.0, 0.0)
    flat, ref, score = _overlapping(K * PLANE, 2 * N * M, 3)  # score begins inside ref
    _rejected('tvae_pose_classify', i['Y'], i['theta'], i['dx'], i['cand'], ref.view(K, C, n, n), o['cls_out'], o['best'],
              o['theta_out'], o['dx_out'], score.view(N, M, 2), None, None, None, o['ws'], *tail)
    _all_sentinels(flat, *o.values())
    _accepted('tvae_pose_classify', i['Y'], i['theta'], i['dx'], i['cand'], i['ref'], *o.values(), *tail)
    assert o['cls_out'].tolist()[2] == 0 and bool((o['yy'] > 0).all())      # image 2 has one live slot, class 0

    # the posterior of those tables
    f64 = lambda: torch.full((N,), SENT_F, dtype=torch.float64, device=DEV)
    e = dict(idx=_sent(N, P, dtype=torch.int32), cls=_sent(N, P, dtype=torch.int32), theta=_sent(N, P), dx=_sent(N, P, 2), w=_sent(N, P),
             resp=_sent(N, M), lse=f64(), r2=f64(), kept=_sent(N))
    tail = (N, n, K, M, A, S, P, 1.0, 0.1, 1.0)
    flat, yy, w = _overlapping(N, N * P, 1)                   # ent_w begins at the last word of yy
    _rejected('tvae_pose_posterior', o['num'], o['pp'], yy, i['cand'], None, i['theta'], i['dx'], e['idx'], e['cls'], e['theta'], e['dx'],
              w.view(N, P), e['resp'], e['lse'], e['r2'], e['kept'], *tail)
    _all_sentinels(flat, *e.values())
    _accepted('tvae_pose_posterior', o['num'], o['pp'], o['yy'], i['cand'], None, i['theta'], i['dx'], *e.values(), *tail)
    assert np.allclose(e['resp'].sum(1).cpu().numpy(), 1.0, atol=1e-5) and bool((e['kept'] > 0).all())


def test_class_average_weighted():
    from tvae import _cluster_lib as CL
    i = _inputs()
    E = 4
    img = torch.tensor([0, 2, 1, 0], dtype=torch.int32, device=DEV)
    th, d, w = torch.zeros(E, device=DEV), torch.zeros(E, 2, device=DEV), torch.ones(E, device=DEV)
    seg = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    wsf = CL.query('tvae_class_average_weighted_ws_floats', E, K, C, n)
    assert wsf > 0
    ws = CL.workspace(wsf, DEV)
    ws.fill_(SENT_F)
    o = dict(avg=_sent(K, C, n, n), wsum=torch.full((K,), SENT_F, dtype=torch.float64, device=DEV), counts=_sent(K, dtype=torch.int32))
    tail = (wsf, N, E, C, n, K, 1.0)
    flat, Y, avg = _overlapping(N * PLANE, K * PLANE, PLANE)  # avg begins at the last image of Y
    _rejected('tvae_class_average_weighted', Y.view(N, C, n, n), img, th, d, w, seg, avg.view(K, C, n, n), o['wsum'], o['counts'], ws,
              *tail)
    _all_sentinels(flat, ws, *o.values())
    _accepted('tvae_class_average_weighted', i['Y'], img, th, d, w, seg, *o.values(), ws, *tail)
    assert o['counts'].tolist() == [2, 2] and o['wsum'].tolist() == [2.0, 2.0]
    assert torch.allclose(o['avg'][0], (i['Y'][0] + i['Y'][2]) / 2, atol=1e-4)      # theta = 0, dx = 0: the images themselves
