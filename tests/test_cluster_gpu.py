"""The clustering half on the GPU: the k-means kernels of libtvae_cluster.so behind their C ABI (every call under guard
bands with replay: out-of-bounds writes, reads beyond the tensors and run-to-run determinism), tvae.cluster.kmeans,
tvae.latent on all three inference branches, extract_latents and the clustering CLIs.

Label acceptance against fp64: the kernels form distances as sum_j (x_j - c_j)^2 in fp32, whose rounding error is at
most (d + 2) * 2^-24 relative to the distance itself; a GPU label g of point n is accepted iff
D64[n][g] <= min_j D64[n][j] * (1 + 4 (d + 2) 2^-24), twice that bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guardband
from conftest import GOLDEN, PKG, load_golden, rel_err, tdict

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 2.0 ** -24
SENT_F, SENT_I = -12345.5, -77


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


def _feature_major(X):
    from tvae import cluster
    return cluster._feature_major(torch.from_numpy(np.ascontiguousarray(X)).to(DEV))


class Lloyd:
    """Device state of R restarts and one guarded assign + update step."""

    def __init__(self, X, C, prev=None, ldx=None, skew=0):
        """ldx / skew: another row stride of Xt and an offset of its first element in floats (default: the padded,
        16-byte aligned layout of tvae.cluster, which takes the kernels' vector loads)."""
        from tvae import _cluster_lib as CL
        self.CL = CL
        self.N, self.d = X.shape
        self.R, self.k = C.shape[:2]
        if ldx is None and not skew:
            self.Xt, self.ldx = _feature_major(X)
        else:
            self.ldx = ldx if ldx is not None else (self.N + 3) // 4 * 4
            assert self.ldx >= self.N
            store = torch.full((self.d * self.ldx + skew,), SENT_F, device=DEV)
            self.Xt = store[skew:].view(self.d, self.ldx)
            self.Xt[:, :self.N] = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV)
        self.C = torch.from_numpy(np.ascontiguousarray(C)).to(DEV)
        self.wsf = CL.query('tvae_kmeans_ws_floats', self.N, self.d, self.k, self.R)
        assert self.wsf > 0
        self.ws = torch.full((self.wsf,), SENT_F, device=DEV)
        self.labels = torch.full((self.R, self.N), -1, dtype=torch.int32, device=DEV)
        if prev is not None:
            self.labels.copy_(torch.from_numpy(prev))
        self.mind2 = torch.full((self.R, self.N), SENT_F, device=DEV)
        self.changed = torch.full((self.R,), SENT_I, dtype=torch.int32, device=DEV)
        self.inertia = torch.full((self.R,), SENT_F, device=DEV)
        self.shift = torch.full((self.R,), SENT_F, device=DEV)
        self.done = torch.zeros(self.R, dtype=torch.int32, device=DEV)

    def assign(self):
        self.CL.call('tvae_kmeans_assign', self.Xt, self.ldx, self.C, self.done, self.labels, self.mind2, self.changed,
                     self.ws, self.wsf, self.N, self.d, self.k, self.R)

    def update(self):
        self.CL.call('tvae_kmeans_update', self.ws, self.wsf, self.done, self.C, self.inertia, self.shift, self.N, self.d,
                     self.k, self.R)

    def counts(self):
        """per-restart cluster sizes from the workspace partials [G][k]"""
        G = self.CL.query('tvae_kmeans_groups', self.N, self.d, self.k)
        per = self.wsf // self.R
        w = self.ws.view(self.R, per)[:, G * self.k * self.d:G * self.k * self.d + G * self.k]
        return w.contiguous().view(torch.int32).view(self.R, G, self.k).sum(1).cpu().numpy()


def _d64(X, C):
    X, C = X.astype(np.float64), C.astype(np.float64)
    return ((X[:, None, :] - C[None, :, :]) ** 2).sum(2) if X.shape[0] * C.shape[0] * X.shape[1] < 3e7 else \
        np.stack([((X - c) ** 2).sum(1) for c in C], 1)


CASES = [(4099, 4, 10, 3), (1000, 100, 37, 2), (777, 206, 3, 1), (5000, 2, 200, 1), (300, 7, 1, 1), (65, 1, 2, 2),
         (70001, 16, 64, 2)]


def _case_data(N, d, k, R):
    rng = np.random.default_rng(1000 * d + k)
    X = rng.standard_normal((N, d)).astype(np.float32)
    C = np.stack([X[rng.permutation(N)[:k]] for _ in range(R)])
    return X, C


@pytest.mark.parametrize('N,d,k,R', CASES)
def test_lloyd_step_against_fp64(N, d, k, R):
    X, C = _case_data(N, d, k, R)
    st = Lloyd(X, C)
    with guardband.GuardedCalls(replay=True):
        st.assign()
        st.update()
    lab = st.labels.cpu().numpy()
    md = st.mind2.cpu().numpy().astype(np.float64)
    Cn = st.C.cpu().numpy()
    counts = st.counts()
    assert np.array_equal(st.changed.cpu().numpy(), np.full(R, N))            # against previous labels of all -1
    for r in range(R):
        D = _d64(X, C[r])
        dmin = D.min(1)
        got = D[np.arange(N), lab[r]]
        ok = got <= dmin * (1 + 4 * (d + 2) * EPS)
        differ = int((lab[r] != D.argmin(1)).sum())
        print(f'case {(N, d, k, R)} restart {r}: outside margin {int((~ok).sum())}, differ from fp64 argmin {differ}')
        assert ok.all()
        assert differ <= 0.005 * N
        assert (np.abs(md[r] - got) <= 2 * (d + 2) * EPS * got).all()
        # from the GPU's own labels
        cnt = np.bincount(lab[r], minlength=k)
        assert cnt.min() > 0
        assert np.array_equal(counts[r], cnt)
        means = np.stack([X[lab[r] == c].astype(np.float64).mean(0) for c in range(k)])
        assert rel_err(Cn[r], means) <= 1e-4
        assert rel_err(st.inertia[r].item(), md[r].sum()) <= 1e-4
        assert rel_err(st.shift[r].item(), ((means - C[r].astype(np.float64)) ** 2).sum()) <= 1e-4
    # second step: the changed count against the true previous labels
    prev = lab.copy()
    with guardband.GuardedCalls(replay=True):
        st.assign()
    lab2 = st.labels.cpu().numpy()
    assert np.array_equal(st.changed.cpu().numpy(), (lab2 != prev).sum(1))
    for r in range(R):
        D = _d64(X, Cn[r])
        assert (D[np.arange(N), lab2[r]] <= D.min(1) * (1 + 4 * (d + 2) * EPS)).all()


@pytest.mark.parametrize('N,d,k,R,ldx,skew', [(4099, 4, 10, 2, 4101, 0), (4099, 4, 10, 2, None, 1),
                                              (33001, 16, 37, 1, 33001, 0)])
def test_unaligned_points_take_the_scalar_loads(N, d, k, R, ldx, skew):
    """The ABI allows any ldx >= N and any 4-byte aligned Xt.  A row stride that is no multiple of 4, or a base that is not
    16-byte aligned, sends the full tiles of the per-cluster sums through the scalar loads; they add the same points in
    the same order as the vector loads, so five Lloyd steps are bitwise those of the aligned layout.  (33001, 16, 37):
    three tiles per group, more than one pair pass.)"""
    X, C = _case_data(N, d, k, R)
    a, b = Lloyd(X, C), Lloyd(X, C, ldx=ldx, skew=skew)
    assert b.Xt.is_contiguous() and (b.ldx % 4 != 0 or b.Xt.data_ptr() % 16 != 0)
    assert a.ldx % 4 == 0 and a.Xt.data_ptr() % 16 == 0
    with guardband.GuardedCalls(replay=True):
        for _ in range(5):
            for st in (a, b):
                st.assign()
                st.update()
    for name in ('labels', 'mind2', 'changed', 'C', 'inertia', 'shift'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.counts(), b.counts())
    lab = b.labels.cpu().numpy()
    for r in range(R):                                                        # and right, not only equal
        means = np.stack([X[lab[r] == c].astype(np.float64).mean(0) for c in range(k)])
        assert rel_err(b.C[r], means) <= 1e-4


def test_duplicate_centroid_takes_lower_index_and_empty_cluster_keeps_centroid():
    X, C = _case_data(4099, 4, 10, 1)
    C = np.concatenate([C, np.zeros((1, 2, 4), np.float32)], 1)               # k = 12
    C[0, 10] = C[0, 3]                                                        # duplicate of cluster 3
    C[0, 11] = 1e3                                                            # wins no point
    st = Lloyd(X, C)
    with guardband.GuardedCalls(replay=True):
        st.assign()
        st.update()
    lab = st.labels.cpu().numpy()[0]
    assert (lab == 3).sum() > 0 and (lab == 10).sum() == 0 and (lab == 11).sum() == 0
    Cn = st.C.cpu().numpy()[0]
    assert np.array_equal(Cn[11].view(np.int32), C[0, 11].view(np.int32))
    assert np.array_equal(Cn[10].view(np.int32), C[0, 10].view(np.int32))
    assert not np.array_equal(Cn[3], C[0, 3])


def test_done_restart_is_not_touched():
    X, C = _case_data(4099, 4, 10, 3)
    st = Lloyd(X, C)
    st.done[1] = 1
    st.labels[1] = SENT_I
    ws0 = st.ws.clone()
    with guardband.GuardedCalls(replay=True):
        st.assign()
        st.update()
    per = st.wsf // 3
    assert torch.equal(st.ws[per:2 * per].view(torch.int32), ws0[per:2 * per].view(torch.int32))
    assert (st.labels[1] == SENT_I).all() and (st.mind2[1] == SENT_F).all()
    assert st.changed[1].item() == SENT_I and st.inertia[1].item() == SENT_F and st.shift[1].item() == SENT_F
    assert np.array_equal(st.C[1].cpu().numpy(), C[1])
    for r in (0, 2):
        assert (st.labels[r] >= 0).all() and st.changed[r].item() == 4099 and st.inertia[r].item() > 0
        assert not np.array_equal(st.C[r].cpu().numpy(), C[r])


@pytest.mark.parametrize('N,d,k', [(8, 4, 9), (300, 257, 3), (2000, 2, 1025)])
def test_unsupported_shapes_are_rejected_untouched(N, d, k):
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    assert CL.query('tvae_kmeans_ws_floats', N, d, k, 1) == 0
    Xt = torch.randn(d, (N + 3) // 4 * 4, device=DEV)
    C = torch.randn(1, k, d, device=DEV)
    labels = torch.full((1, N), SENT_I, dtype=torch.int32, device=DEV)
    mind2, ws = torch.full((1, N), SENT_F, device=DEV), torch.full((1 << 16,), SENT_F, device=DEV)
    changed, done = torch.full((1,), SENT_I, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    inertia, shift = torch.full((1,), SENT_F, device=DEV), torch.full((1,), SENT_F, device=DEV)
    C0 = C.clone()
    g = guardband.GuardedCalls(replay=True)
    with g:                                      # the guard also checks that a rejected call left every tensor alone
        with pytest.raises(TvaeHipError):
            CL.call('tvae_kmeans_assign', Xt, Xt.shape[1], C, done, labels, mind2, changed, ws, ws.numel(), N, d, k, 1)
        with pytest.raises(TvaeHipError):
            CL.call('tvae_kmeans_update', ws, ws.numel(), done, C, inertia, shift, N, d, k, 1)
        if d > 256:
            with pytest.raises(TvaeHipError):
                CL.call('tvae_kmeans_mindist', Xt, Xt.shape[1], C[0, :1].contiguous(), mind2, N, d, 1)
    assert g.calls >= 2 and not g.violations
    assert (labels == SENT_I).all() and (mind2 == SENT_F).all() and (ws == SENT_F).all() and torch.equal(C, C0)
    assert changed.item() == SENT_I and inertia.item() == SENT_F and shift.item() == SENT_F


def test_restart_does_not_depend_on_the_batch():
    X, C = _case_data(4099, 4, 10, 3)
    a, b = Lloyd(X, C), Lloyd(X, C[:1])
    with guardband.GuardedCalls(replay=True):
        for _ in range(5):
            for st in (a, b):
                st.assign()
                st.update()
    for name in ('labels', 'C', 'inertia', 'mind2', 'shift', 'changed'):
        assert torch.equal(getattr(a, name)[0], getattr(b, name)[0]), name


# ---- tvae.cluster.kmeans ------------------------------------------------------------------------------------------------
def _blobs():
    rng = np.random.default_rng(7)
    k, d, m = 6, 4, 50
    means = 20 * rng.standard_normal((k, d))
    X = (means[:, None, :] + rng.standard_normal((k, m, d))).reshape(k * m, d).astype(np.float32)
    y = np.repeat(np.arange(k), m)
    return X, y, X[::m].copy()


def test_kmeans_separated_blobs():
    from tvae import cluster
    X, y, init = _blobs()
    Xd = torch.from_numpy(X).to(DEV)
    with guardband.GuardedCalls(replay=True):
        res = cluster.kmeans(Xd, 6, init=torch.from_numpy(init)[None].to(DEV))
    assert np.array_equal(res.labels.cpu().numpy(), y) and res.labels.dtype == torch.int64
    assert res.n_iter <= 3 and res.best == 0
    X64 = X.astype(np.float64)
    means = np.stack([X64[y == c].mean(0) for c in range(6)])
    inertia64 = ((X64 - means[y]) ** 2).sum()
    print('blob inertia', res.inertia, inertia64)
    assert abs(inertia64 - 1067.8054) < 1e-3
    assert rel_err(res.inertia, inertia64) <= 1e-4
    assert rel_err(res.centers, means) <= 1e-4
    D = _d64(X, res.centers.cpu().numpy())
    assert np.array_equal(D.argmin(1), res.labels.cpu().numpy())


def test_kmeans_picks_the_restart_of_lowest_inertia():
    from tvae import cluster
    X, y, good = _blobs()
    bad = [X[i * 6:i * 6 + 6] for i in range(3)]                              # all six seeds inside blob 0
    init = torch.from_numpy(np.stack([bad[0], bad[1], good, bad[2]])).to(DEV)
    Xd = torch.from_numpy(X).to(DEV)
    with guardband.GuardedCalls(replay=True):
        res = cluster.kmeans(Xd, 6, init=init)
        one = cluster.kmeans(Xd, 6, init=init[2:3])
    assert res.best == 2 and int(torch.argmin(res.all_inertia)) == 2 and res.all_inertia.shape == (4,)
    assert (res.all_inertia[[0, 1, 3]] > res.all_inertia[2]).all()
    assert torch.equal(res.labels, one.labels) and torch.equal(res.centers, one.centers)
    assert res.inertia == one.inertia and res.n_iter == one.n_iter
    assert np.array_equal(res.labels.cpu().numpy(), y)


def test_kmeans_plusplus():
    from tvae import _cluster_lib as CL, cluster
    X, _ = _case_data(4099, 4, 10, 1)
    Xd = torch.from_numpy(X).to(DEV)
    with guardband.GuardedCalls(replay=True):
        C1 = cluster.kmeans_plusplus(Xd, 10, 3, seed=5)
        C2 = cluster.kmeans_plusplus(Xd, 10, 3, seed=5)
    assert torch.equal(C1, C2) and not torch.equal(C1[0], C1[1])
    rows = {r.tobytes() for r in X}
    assert all(c.tobytes() in rows for c in C1.cpu().numpy().reshape(-1, 4))
    # the D^2 step against fp64
    Xt, ldx = _feature_major(X)
    cn = Xd[[17, 4000]].contiguous()
    D = torch.full((2, 4099), float('inf'), device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_kmeans_mindist', Xt, ldx, cn, D, 4099, 4, 2)
    D64 = _d64(X, X[[17, 4000]]).T
    assert (np.abs(D.cpu().numpy() - D64) <= 2 * (4 + 2) * EPS * D64).all()
    prev = torch.full((2, 4099), 0.5, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_kmeans_mindist', Xt, ldx, cn, prev, 4099, 4, 2)
    assert torch.equal(prev, torch.minimum(D, torch.full_like(D, 0.5)))


def test_kmeans_plusplus_recovers_blobs():
    from tvae import cluster
    X, y, _ = _blobs()
    Xd = torch.from_numpy(X).to(DEV)
    with guardband.GuardedCalls(replay=True):
        a = cluster.kmeans(Xd, 6, n_init=8, seed=11)
        b = cluster.kmeans(Xd, 6, n_init=8, seed=11)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.centers, b.centers) and a.inertia == b.inertia
    assert torch.equal(a.all_inertia, b.all_inertia)
    _, acc = cluster.cluster_acc(y, a.labels.cpu().numpy())
    assert acc == 1.0


# ---- latents ------------------------------------------------------------------------------------------------------------
def _attention_encoder(fx):
    import src.models as M
    n, cin, zd, C, k, p, R, refine, normal = [int(v) for v in fx['cfg']][:9]
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(
        n, cin, zd, kernels_num=C, kernels_size=k, padding=p, groupconv=R, rot_refinement=bool(refine),
        theta_prior=float(fx['theta_prior']), normal_prior_over_r=bool(normal))
    enc.load_state_dict(tdict(fx, 'p.'))
    return enc.to(DEV), n


def test_extract_latents_is_the_concatenation_of_get_latent():
    from tvae import latent, tables
    fx = load_golden('get_latent_P8_28')
    enc, n = _attention_encoder(fx)
    y4 = torch.from_numpy(fx['y'])
    y = torch.cat([y4, torch.roll(y4, (2, -3), (2, 3)), torch.roll(y4[:2], (-4, 1), (2, 3))]).to(DEV)
    assert y.shape[0] == 10
    x = torch.from_numpy(tables.image_coords(n)).to(DEV)
    with guardband.GuardedCalls(replay=True):
        zc, th, dx = latent.extract_latents(y, enc, x, 'attention', 'attention+offsets', minibatch_size=4)
        parts = [latent.get_latent(x, y[a:b], enc, 'attention', 'attention+offsets', DEV, n)
                 for a, b in ((0, 4), (4, 8), (8, 10))]
    assert zc.shape == (10, 4) and th.shape == (10, 1) and dx.shape == (10, 2)
    for got, i in ((zc, 0), (th, 1), (dx, 2)):
        assert torch.equal(got, torch.cat([p[i] for p in parts]))
    # the first slice is the golden's own batch: the unchanged function still meets the reference
    assert rel_err(zc[:4], fx['z_content']) < 1e-4 and rel_err(th[:4], fx['theta_mu']) < 1e-4
    assert rel_err(dx[:4], fx['dx']) < 1e-4
    # the 6-argument signature of the particles / galaxy / dsprites scripts
    with guardband.GuardedCalls(replay=True):
        six = latent.get_latent(x, y[:4], enc, 'attention', 'attention+offsets', DEV)
    assert all(torch.equal(a, b) for a, b in zip(six, parts[0]))


@pytest.mark.parametrize('name', ['get_latent_unimodal_unimodal', 'get_latent_attention_unimodal_gc4',
                                  'get_latent_attention_unimodal_gc0'])
def test_get_latent_secondary_branches_golden(name):
    """The two secondary branches against the reference's clustering_mnist.get_latent (goldens from the real function,
    tests/golden/make_goldens_clustering.py)."""
    import src.models as M
    from tvae import latent, tables
    fx = load_golden(name)
    n, zd, gc = [int(v) for v in fx['cfg']]
    if 'unimodal_unimodal' in name:
        enc, t_inf = M.InferenceNetwork_UnimodalTranslation_UnimodalRotation(n * n, zd + 3, 32, num_layers=2), 'unimodal'
    else:
        enc, t_inf = M.InferenceNetwork_AttentionTranslation_UnimodalRotation(n, 1, zd, kernels_num=8, groupconv=gc), 'attention'
    enc.load_state_dict(tdict(fx, 'p.'))
    enc = enc.to(DEV)
    x = torch.from_numpy(tables.image_coords(n)).to(DEV)
    y = torch.from_numpy(fx['y']).to(DEV)
    with guardband.GuardedCalls(replay=True):
        zc, th, dx = latent.get_latent(x, y, enc, t_inf, 'unimodal', DEV, n)
        ex = latent.extract_latents(torch.cat([y, y[:2]]), enc, x, t_inf, 'unimodal', minibatch_size=4)
    assert tuple(zc.shape) == tuple(fx['z_content'].shape) == (4, 2 * zd)
    assert tuple(th.shape) == tuple(fx['theta_mu'].shape) == (4, 1) and tuple(dx.shape) == tuple(fx['dx'].shape) == (4, 2)
    for got, key in ((zc, 'z_content'), (th, 'theta_mu'), (dx, 'dx')):
        print(name, key, rel_err(got, fx[key]))
        assert rel_err(got, fx[key]) <= 1e-4, key
    for got, want in zip(ex, (zc, th, dx)):
        assert torch.equal(got[:4], want) and got.shape[0] == 6


# ---- command lines ------------------------------------------------------------------------------------------------------
def test_clustering_mnist_cli(tmp_path):
    import src.models as M
    from tvae import cluster
    rng = np.random.default_rng(0)
    n, zd, N = 32, 2, 24
    os.makedirs(tmp_path / 'data' / 'mnist_U')
    plain = np.zeros((N, 28, 28), np.uint8)
    labels = np.arange(N) % 3
    for i in range(N):                                     # three classes of bars / blocks
        c = labels[i]
        plain[i, 6 + 5 * c:12 + 5 * c, 4:24 - 6 * c] = 200 + rng.integers(0, 50)
    imgs = np.zeros((N, n, n), np.uint8)
    shifts = rng.integers(-2, 3, (N, 2))
    for i in range(N):
        imgs[i] = np.roll(np.pad(plain[i], 2), tuple(shifts[i]), (0, 1))
    np.save(tmp_path / 'data' / 'mnist_U' / 'images_test.npy', imgs)
    tr = np.concatenate([rng.uniform(-3, 3, (N, 1)), shifts[:, ::-1] * (2.0 / (n - 1))], 1)
    np.save(tmp_path / 'data' / 'mnist_U' / 'transforms_test.npy', tr)
    torch.save((torch.from_numpy(plain), torch.from_numpy(labels)), tmp_path / 'test.pt')
    torch.manual_seed(4)
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(
        n, 1, zd, kernels_num=8, kernels_size=n, padding=4, groupconv=8, rot_refinement=True, theta_prior=np.pi,
        normal_prior_over_r=False)
    os.makedirs(tmp_path / 'model')
    torch.save(enc, tmp_path / 'model' / 'inference.sav')
    cmd = [sys.executable, os.path.join(PKG, 'clustering_mnist.py'), '--dataset', 'mnist-U', '--clustering', 'k-means',
           '--n-clusters', '3', '--n-init', '4', '--seed', '0', '--image-dim', str(n), '--minibatch-size', '10',
           '--path-to-encoder', 'model/inference.sav', '--path-to-mnist-test', 'test.pt']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'figures of the reference are not built' in r.stderr
    out = tmp_path / 'model'
    lines = open(out / 'results.txt').read().splitlines()
    assert lines[0] == 'using the encoder model from model/inference.sav' and lines[1] == ''
    assert lines[2].startswith('The accuracy for clustering is ')
    assert lines[3].startswith('The circular correlation for the rotation is ')
    assert lines[4].startswith('The Pearson correlation for the x and y values in the translation is [') and len(lines) == 5
    shapes = {f: np.load(out / (f + '.npy')).shape for f in ('latents', 'rotations', 'translations', 'clusters')}
    assert shapes == dict(latents=(N, 2 * zd), rotations=(N, 1), translations=(N, 2), clusters=(N,))
    clusters = np.load(out / 'clusters.npy')
    assert set(clusters.tolist()) <= {0, 1, 2}
    _, acc = cluster.cluster_acc(labels, clusters)
    assert float(lines[2].split(' is ')[1]) == acc
    assert np.isfinite(np.load(out / 'latents.npy')).all()


def test_clustering_particles_cli_from_mrcs(tmp_path):
    """clustering_particles.py on the reference-written stack of tests/golden (5 images of 6 x 7, cropped to 6 x 6), MLP
    encoder, agglomerative clustering on the host: results.txt without accuracy or correlation lines."""
    import src.models as M
    torch.manual_seed(2)
    enc = M.InferenceNetwork_UnimodalTranslation_UnimodalRotation(36, 2 + 3, 16, num_layers=2)
    torch.save(enc, tmp_path / 'inference.sav')
    cmd = [sys.executable, os.path.join(PKG, 'clustering_particles.py'), '--test-path', os.path.join(GOLDEN, 'stack_ref.mrcs'),
           '--crop', '6', '--t-inf', 'unimodal', '--r-inf', 'unimodal', '--clustering', 'agglomerative', '--n-clusters', '2',
           '--path-to-encoder', str(tmp_path / 'inference.sav'), '--out-dir', str(tmp_path / 'out')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(tmp_path / 'out' / 'results.txt').read()
    assert text == 'using the encoder model from {}\n\n'.format(tmp_path / 'inference.sav')
    assert np.load(tmp_path / 'out' / 'clusters.npy').shape == (5,) and np.load(tmp_path / 'out' / 'latents.npy').shape == (5, 4)
    assert sorted(set(np.load(tmp_path / 'out' / 'clusters.npy').tolist())) == [0, 1]
