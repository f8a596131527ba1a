"""Ward agglomerative clustering on the GPU: tvae_ward_nn and tvae_ward_merge behind their C ABI (every call under guard
bands with replay), tvae.cluster.ward_linkage against scipy's fp64 `ward`, ward_cut / agglomerative against sklearn,
and the TVAE_WARD switch of the clustering command line.

Neighbour acceptance against fp64: w(i,j) = (cnt_i cnt_j) / (cnt_i + cnt_j) * sum_f (c_if - c_jf)^2 is formed in fp32;
the sum carries at most (d + 2) roundings relative to itself (the k-means label rule of test_cluster_gpu.py) and the
size factor two more, so nn[i] = g is accepted iff w64(i,g) <= min_j w64(i,j) * (1 + 4 (d + 4) 2^-24), and nd[i] has to
sit within the same relative bound of w64(i, nn[i]).  Dendrogram heights: 1e-4 relative, the parity tolerance of this
project."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guardband
from conftest import GOLDEN, PKG

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


def same_partition(a, b):
    a, b = np.asarray(a).tolist(), np.asarray(b).tolist()
    return len(set(zip(a, b))) == len(set(a)) == len(set(b))


# ---- tvae_ward_nn ---------------------------------------------------------------------------------------------------------
def _layout(X, ldc=None, skew=0):
    """X [M][d] -> contiguous Ct [d][ldc] on the device whose first element sits `skew` floats into its allocation; the
    padding holds a sentinel."""
    M, d = X.shape
    ldc = (M + 3) // 4 * 4 if ldc is None else ldc
    store = torch.full((d * ldc + skew,), SENT_F, device=DEV)
    Ct = store[skew:].view(d, ldc)
    Ct[:, :M] = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV)
    return Ct, ldc


def _run_nn(X, cnt, ldc=None, skew=0):
    from tvae import _cluster_lib as CL
    M, d = X.shape
    Ct, ldc = _layout(X, ldc, skew)
    wsf = CL.query('tvae_ward_nn_ws_floats', M, d)
    assert wsf == 2 * CL.query('tvae_ward_nn_splits', M, d) * M > 0
    ws = torch.full((wsf,), SENT_F, device=DEV)
    nn = torch.full((M,), SENT_I, dtype=torch.int32, device=DEV)
    nd = torch.full((M,), SENT_F, device=DEV)
    with guardband.GuardedCalls(replay=True):
        CL.call('tvae_ward_nn', Ct, ldc, torch.from_numpy(cnt).to(DEV), nn, nd, ws, wsf, M, d)
    return Ct, nn.cpu().numpy(), nd.cpu().numpy()


def _w64(X, cnt):
    X, n = X.astype(np.float64), cnt.astype(np.float64)
    if X.shape[0] * X.shape[0] * X.shape[1] < 3e7:
        D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(2)
    else:
        D = np.stack([((X - x) ** 2).sum(1) for x in X])
    W = n[:, None] * n[None, :] / (n[:, None] + n[None, :]) * D
    np.fill_diagonal(W, np.inf)
    return W


NN_SHAPES = [(257, 2), (1000, 100), (65, 1), (40, 256), (4099, 4)]


@pytest.mark.parametrize('M,d', NN_SHAPES)
def test_nn_against_fp64_in_both_layouts(M, d):
    rng = np.random.default_rng(100 * d + M)
    X = rng.standard_normal((M, d)).astype(np.float32)
    cnt = rng.integers(1, 51, M).astype(np.float32)
    W = _w64(X, cnt)
    wmin = W.min(1)
    tol = 4 * (d + 4) * EPS
    Ct_a, nn_a, nd_a = _run_nn(X, cnt)
    odd = M + 1 if (M + 1) % 4 else M + 3
    Ct_b, nn_b, nd_b = _run_nn(X, cnt, ldc=odd, skew=1)
    assert Ct_a.shape[1] % 4 == 0 and Ct_a.data_ptr() % 16 == 0
    assert Ct_b.is_contiguous() and Ct_b.shape[1] % 4 != 0 and Ct_b.data_ptr() % 16 != 0
    for name, nn, nd in (('aligned', nn_a, nd_a), ('scalar', nn_b, nd_b)):
        assert ((nn >= 0) & (nn < M) & (nn != np.arange(M))).all(), name
        got = W[np.arange(M), nn]
        differ = int((nn != W.argmin(1)).sum())
        worst = float((got / wmin).max() - 1)
        nd_err = float((np.abs(nd - got) / got).max())
        print(f'nn {(M, d)} {name}: differ from fp64 argmin {differ}, worst w64 ratio - 1 = {worst:.3e}, '
              f'nd error {nd_err:.3e}, bound {tol:.3e}')
        assert (got <= wmin * (1 + tol)).all(), name
        assert (np.abs(nd - got) <= tol * got).all(), name
    # the scalar instance does the same arithmetic in the same order
    assert np.array_equal(nn_a, nn_b) and np.array_equal(nd_a.view(np.int32), nd_b.view(np.int32))


def test_nn_duplicate_rows_go_to_the_lowest_index_and_w_is_symmetric():
    rng = np.random.default_rng(5)
    M, d = 700, 3
    X = rng.standard_normal((M, d)).astype(np.float32)
    cnt = rng.integers(1, 51, M).astype(np.float32)
    for i in (300, 650):                                   # three copies of slot 7, sizes included
        X[i], cnt[i] = X[7], cnt[7]
    _, nn, nd = _run_nn(X, cnt)
    assert nn[7] == 300 and nn[300] == 7 and nn[650] == 7 and nn[nn[7]] == 7
    assert nd[7] == 0 and nd[300] == 0 and nd[650] == 0
    # bitwise symmetry: a reciprocal pair reports the same distance from both sides; the global minimum is reciprocal
    i = np.arange(M)
    mutual = nn[nn] == i
    assert mutual.sum() >= 2
    assert np.array_equal(nd[mutual].view(np.int32), nd[nn[mutual]].view(np.int32))
    # the tie rule across column tiles and column ranges: identical points everywhere -> everybody names slot 0, slot 0 names 1
    M2 = 1500
    _, nn2, nd2 = _run_nn(np.ones((M2, 2), np.float32), np.ones(M2, np.float32))
    assert nn2[0] == 1 and (nn2[1:] == 0).all() and (nd2 == 0).all()


# ---- tvae_ward_merge ------------------------------------------------------------------------------------------------------
class MergeState:
    def __init__(self, C, cnt, ids, hmax, nn, N, base, cap):
        from tvae import _cluster_lib as CL
        self.CL = CL
        self.M, self.d = C.shape
        M, d = self.M, self.d
        self.N, self.base, self.cap = N, base, cap
        self.ld_in, self.ld_out = (M + 3) // 4 * 4, M + 5
        self.C_in = torch.zeros(d, self.ld_in, dtype=torch.float64, device=DEV)
        self.C_in[:, :M] = torch.from_numpy(np.ascontiguousarray(C.T)).to(DEV)
        self.cnt_in = torch.from_numpy(cnt.astype(np.float32)).to(DEV)
        self.id_in = torch.from_numpy(ids.astype(np.int32)).to(DEV)
        self.hmax_in = torch.from_numpy(hmax.astype(np.float64)).to(DEV)
        self.nn = torch.from_numpy(nn.astype(np.int32)).to(DEV)
        self.C_out = torch.full((d, self.ld_out), SENT_F, dtype=torch.float64, device=DEV)
        self.Ct_out = torch.full((d, self.ld_out), SENT_F, device=DEV)
        self.cnt_out = torch.full((M,), SENT_F, device=DEV)
        self.id_out = torch.full((M,), SENT_I, dtype=torch.int32, device=DEV)
        self.hmax_out = torch.full((M,), SENT_F, dtype=torch.float64, device=DEV)
        self.rec_ids = torch.full((cap, 2), SENT_I, dtype=torch.int32, device=DEV)
        self.rec_hs = torch.full((cap, 2), SENT_F, dtype=torch.float64, device=DEV)
        self.m_out = torch.full((1,), SENT_I, dtype=torch.int32, device=DEV)
        self.ws = torch.full((max(2 * M, 8),), SENT_I, dtype=torch.int32, device=DEV)

    def outputs(self):
        return (self.C_out, self.Ct_out, self.cnt_out, self.id_out, self.hmax_out, self.rec_ids, self.rec_hs, self.m_out,
                self.ws)

    def call(self, M=None, d=None):
        self.CL.call('tvae_ward_merge', self.C_in, self.ld_in, self.cnt_in, self.id_in, self.hmax_in, self.nn, self.C_out,
                     self.Ct_out, self.ld_out, self.cnt_out, self.id_out, self.hmax_out, self.rec_ids, self.rec_hs, self.m_out,
                     self.ws, self.ws.numel(), self.M if M is None else M, self.d if d is None else d, self.N, self.base,
                     self.cap)


def _merge_reference(C, cnt, ids, hmax, nn, N, base):
    """The round in numpy fp64: (survivor columns, cnt, ids, hmax, records [(id_i, id_j, h, size)])."""
    M = len(cnt)
    i = np.arange(M)
    mutual = nn[nn] == i
    lead = mutual & (i < nn)
    keep = ~mutual | lead
    C2, cnt2, ids2, h2 = C.copy(), cnt.astype(np.float64).copy(), ids.copy(), hmax.copy()
    rec = []
    for r, a in enumerate(np.nonzero(lead)[0]):
        b = nn[a]
        na, nb = float(cnt[a]), float(cnt[b])
        C2[a] = (na * C[a] + nb * C[b]) / (na + nb)
        h = max(np.sqrt(2 * (na * nb / (na + nb)) * ((C[a] - C[b]) ** 2).sum()), hmax[a], hmax[b])
        rec.append((ids[a], ids[b], h, na + nb))
        cnt2[a], ids2[a], h2[a] = na + nb, N + base + r, h
    return C2[keep], cnt2[keep], ids2[keep], h2[keep], rec


def _check_merge(st, C, cnt, ids, hmax, nn):
    Cs, cnts, idss, hs, rec = _merge_reference(C, cnt, ids, hmax, nn, st.N, st.base)
    m = len(cnts)
    assert st.m_out.item() == m
    got_C = st.C_out.cpu().numpy()
    assert np.allclose(got_C[:, :m].T, Cs, rtol=1e-13, atol=1e-13)
    assert np.array_equal(st.Ct_out.cpu().numpy()[:, :m], got_C[:, :m].astype(np.float32))
    assert np.array_equal(st.cnt_out.cpu().numpy()[:m], cnts.astype(np.float32))
    assert np.array_equal(st.id_out.cpu().numpy()[:m], idss)
    assert np.allclose(st.hmax_out.cpu().numpy()[:m], hs, rtol=1e-13, atol=0)
    # nothing behind the survivors, no record outside [base, base + merges)
    assert (got_C[:, m:] == SENT_F).all() and (st.Ct_out[:, m:] == SENT_F).all() and (st.cnt_out[m:] == SENT_F).all()
    assert (st.id_out[m:] == SENT_I).all() and (st.hmax_out[m:] == SENT_F).all()
    ri, rh = st.rec_ids.cpu().numpy(), st.rec_hs.cpu().numpy()
    lo, hi = st.base, st.base + len(rec)
    assert (ri[:lo] == SENT_I).all() and (ri[hi:] == SENT_I).all() and (rh[:lo] == SENT_F).all() and (rh[hi:] == SENT_F).all()
    assert np.array_equal(ri[lo:hi], np.array([(a, b) for a, b, _, _ in rec]).reshape(-1, 2))
    assert np.allclose(rh[lo:hi], np.array([(h, s) for _, _, h, s in rec]).reshape(-1, 2), rtol=1e-13, atol=0)
    return rec


def test_merge_hand_made_round():
    """Slots 0 <-> 2 and 3 <-> 5 are reciprocal; 1 -> 0, 4 -> 3 and 6 -> 4 form chains into them (no cycle longer than two), 7
    names 6 and nobody names 7.  Slot 2 carries an hmax above the height of its merge: the record is clamped to it."""
    rng = np.random.default_rng(3)
    M, d, N, base, cap = 8, 3, 50, 10, 49
    C = rng.standard_normal((M, d))
    cnt = np.arange(1, M + 1)
    ids = np.array([7, 3, 60, 12, 5, 61, 9, 30])
    hmax = np.array([0, 0, 100.0, 0.25, 0, 0.5, 0, 0])
    nn = np.array([2, 0, 0, 5, 3, 3, 4, 6])
    st = MergeState(C, cnt, ids, hmax, nn, N, base, cap)
    with guardband.GuardedCalls(replay=True):
        st.call()
    rec = _check_merge(st, C, cnt, ids, hmax, nn)
    assert st.m_out.item() == 6
    assert st.id_out.cpu().numpy()[:6].tolist() == [N + base, 3, N + base + 1, 5, 9, 30]       # ascending old slot order
    assert [(a, b) for a, b, _, _ in rec] == [(7, 60), (12, 61)]
    rh = st.rec_hs.cpu().numpy()[base:base + 2]
    assert rh[0].tolist() == [100.0, 4.0]                                                      # the clamp
    assert np.sqrt(2 * (1 * 3 / 4) * ((C[0] - C[2]) ** 2).sum()) < 100
    h1 = np.sqrt(2 * (4 * 6 / 10) * ((C[3] - C[5]) ** 2).sum())
    assert h1 > 0.5 and abs(rh[1, 0] - h1) <= 1e-13 * h1 and rh[1, 1] == 10
    assert st.hmax_out.cpu().numpy()[[0, 2]].tolist() == [100.0, rh[1, 0]]


def test_merge_of_a_real_round_over_several_scan_chunks():
    """M = 2500 (three chunks of the scan), d = 20 (more features than feature slices), nn from tvae_ward_nn itself.  How
    many pairs are reciprocal depends on the data (few in 20 dimensions); the progress argument guarantees one."""
    rng = np.random.default_rng(11)
    M, d, N, base = 2500, 20, 4000, 1500
    C = rng.standard_normal((M, d))
    cnt = rng.integers(1, 51, M)
    _, nn, _ = _run_nn(C.astype(np.float32), cnt.astype(np.float32))
    ids = rng.permutation(N + base)[:M]
    hmax = np.abs(rng.standard_normal(M)) * (rng.random(M) < 0.3)
    st = MergeState(C, cnt, ids, hmax, nn, N, base, N - 1)
    with guardband.GuardedCalls(replay=True):
        st.call()
    rec = _check_merge(st, C, cnt, ids, hmax, nn)
    assert 1 <= len(rec) <= M // 2


def test_merge_of_many_pairs_over_several_scan_chunks():
    """The same shape with a hand-made nn: 1800 randomly chosen slots form 900 reciprocal pairs, each of the other 700
    names a paired slot (never reciprocal: that slot names its partner).  900 records, ranks by ascending lower slot
    across the three chunks of the scan."""
    rng = np.random.default_rng(12)
    M, d, N, base = 2500, 20, 4000, 1500
    C = rng.standard_normal((M, d))
    cnt = rng.integers(1, 51, M)
    perm = rng.permutation(M)
    a, b, rest = perm[:900], perm[900:1800], perm[1800:]
    nn = np.empty(M, np.int64)
    nn[a], nn[b] = b, a
    nn[rest] = perm[rng.integers(0, 1800, rest.size)]
    ids = rng.permutation(N + base)[:M]
    hmax = np.abs(rng.standard_normal(M)) * (rng.random(M) < 0.3)
    st = MergeState(C, cnt, ids, hmax, nn, N, base, N - 1)
    with guardband.GuardedCalls(replay=True):
        st.call()
    rec = _check_merge(st, C, cnt, ids, hmax, nn)
    assert len(rec) == 900 and st.m_out.item() == M - 900


@pytest.mark.parametrize('M,d', [(1, 3), (8, 257)])
def test_rejected_calls_leave_everything_untouched(M, d):
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    st = MergeState(np.zeros((8, 3)), np.ones(8), np.arange(8), np.zeros(8), np.array([1, 0, 3, 2, 5, 4, 7, 6]), 50, 0, 49)
    before = [t.clone() for t in st.outputs()]
    Ct = torch.randn(3, 8, device=DEV)
    nn = torch.full((8,), SENT_I, dtype=torch.int32, device=DEV)
    nd, ws = torch.full((8,), SENT_F, device=DEV), torch.full((4096,), SENT_F, device=DEV)
    g = guardband.GuardedCalls(replay=True)
    with g:                                      # the guard also checks that a rejected call left every tensor alone
        with pytest.raises(TvaeHipError):
            st.call(M=M, d=d)
        with pytest.raises(TvaeHipError):
            CL.call('tvae_ward_nn', Ct, 8, st.cnt_in, nn, nd, ws, ws.numel(), M, d)
        with pytest.raises(TvaeHipError):        # a workspace that is too small
            CL.call('tvae_ward_nn', Ct, 8, st.cnt_in, nn, nd, ws, 3, 8, 3)
        with pytest.raises(TvaeHipError):        # more merges possible than the record arrays hold
            CL.call('tvae_ward_merge', st.C_in, st.ld_in, st.cnt_in, st.id_in, st.hmax_in, st.nn, st.C_out, st.Ct_out,
                    st.ld_out, st.cnt_out, st.id_out, st.hmax_out, st.rec_ids, st.rec_hs, st.m_out, st.ws, st.ws.numel(),
                    8, 3, 50, 46, 49)
    assert g.calls == 4 and not g.violations
    for a, b in zip(st.outputs(), before):
        assert torch.equal(a, b)
    assert (nn == SENT_I).all() and (nd == SENT_F).all() and (ws == SENT_F).all()


# ---- ward_linkage ---------------------------------------------------------------------------------------------------------
def _input(kind, N, d, seed):
    rng = np.random.default_rng(seed)
    if kind == 'normal':
        return rng.standard_normal((N, d)).astype(np.float32)
    if kind == 'uniform':
        return rng.uniform(-1, 1, (N, d)).astype(np.float32)
    return (rng.standard_normal((N, d)) + 100).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _linkages(kind, N, d, seed):
    """(X, GPU WardResult, scipy's fp64 Z): computed once per input, shared by the tests below, never modified."""
    from scipy.cluster.hierarchy import ward
    from tvae import cluster
    X = _input(kind, N, d, seed)
    with guardband.GuardedCalls(replay=True):
        res = cluster.ward_linkage(torch.from_numpy(X).to(DEV))
    return X, res, ward(X.astype(np.float64))


LINKAGE_INPUTS = [('normal', 257, 2, 0), ('normal', 300, 4, 1), ('normal', 511, 16, 2), ('normal', 130, 50, 3),
                  ('normal', 2000, 2, 4), ('normal', 64, 1, 6), ('normal', 40, 256, 9), ('uniform', 3000, 2, 7),
                  ('offset', 300, 4, 10), ('normal', 2, 3, 2), ('normal', 3, 3, 3), ('normal', 5, 3, 5)]


@pytest.mark.parametrize('kind,N,d,seed', LINKAGE_INPUTS)
def test_dendrogram_is_scipys(kind, N, d, seed):
    X, res, Zr = _linkages(kind, N, d, seed)
    Z = res.Z
    assert Z.dtype == np.float64 and Z.shape == (N - 1, 4) and 1 <= res.n_rounds <= N - 1
    herr = float((np.abs(Z[:, 2] - Zr[:, 2]) / Zr[:, 2]).max())
    wrong = int((Z[:, [0, 1, 3]] != Zr[:, [0, 1, 3]]).any(1).sum())
    print(f'ward {kind} {(N, d, seed)}: {res.n_rounds} rounds, rows that differ from scipy {wrong}, height error {herr:.3e}')
    assert np.array_equal(Z[:, [0, 1, 3]], Zr[:, [0, 1, 3]])
    assert herr <= 1e-4
    assert (np.diff(Z[:, 2]) >= 0).all() and (Z[:, 0] < Z[:, 1]).all()


def test_ties_and_few_merges_per_round():
    from scipy.cluster.hierarchy import fcluster, ward
    from tvae import cluster
    B = np.random.default_rng(8).standard_normal((100, 2))
    X = np.concatenate([B, B[:40], B[:10]]).astype(np.float32)
    with guardband.GuardedCalls(replay=True):
        res = cluster.ward_linkage(torch.from_numpy(X).to(DEV))
    Z, Zr = res.Z, ward(X.astype(np.float64))
    assert int((Z[:, 2] == 0).sum()) == 50 and res.n_rounds <= len(X) - 1
    assert np.allclose(np.sort(Z[:, 2]), np.sort(Zr[:, 2]), rtol=1e-4, atol=1e-6)
    assert (np.diff(Z[:, 2]) >= 0).all()
    for k in (2, 5, 20, 100):
        got = cluster.ward_cut(Z, k)
        assert same_partition(got, fcluster(Zr, k, 'maxclust')), k
        try:
            from sklearn.cluster import AgglomerativeClustering
        except ImportError:
            continue
        want = AgglomerativeClustering(n_clusters=k, linkage='ward', compute_full_tree=True).fit_predict(X)
        assert same_partition(got, want), k
    # geometric spacing: the nearest-neighbour graph is a chain and a round merges few pairs
    P = (1.5 ** np.arange(40))[:, None].astype(np.float32)
    with guardband.GuardedCalls(replay=True):
        res = cluster.ward_linkage(torch.from_numpy(P).to(DEV))
    print('geometric chain:', res.n_rounds, 'rounds')
    assert res.n_rounds <= 39
    assert np.array_equal(res.Z[:, [0, 1, 3]], ward(P.astype(np.float64))[:, [0, 1, 3]])


CUT_INPUTS = [('normal', 300, 4, 1), ('normal', 257, 2, 0), ('normal', 130, 50, 3)]


@pytest.mark.parametrize('kind,N,d,seed', CUT_INPUTS)
def test_cut_partition_is_the_maxclust_partition(kind, N, d, seed):
    from scipy.cluster.hierarchy import fcluster
    from tvae import cluster
    X, res, Zr = _linkages(kind, N, d, seed)
    for k in (1, 2, 5, 10, N):
        assert same_partition(cluster.ward_cut(res.Z, k), fcluster(Zr, k, 'maxclust')), k


@pytest.mark.parametrize('kind,N,d,seed', CUT_INPUTS)
def test_agglomerative_labels_are_sklearns(kind, N, d, seed):
    sk = pytest.importorskip('sklearn.cluster')
    from tvae import cluster
    X, res, _ = _linkages(kind, N, d, seed)
    Xd = torch.from_numpy(X).to(DEV)
    for k in (1, 2, 5, 10, N):
        want = sk.AgglomerativeClustering(n_clusters=k, linkage='ward', compute_full_tree=True).fit_predict(X)
        assert np.array_equal(cluster.ward_cut(res.Z, k), want), k
    with guardband.GuardedCalls(replay=True):
        got = cluster.agglomerative(Xd, 5)
    want = sk.AgglomerativeClustering(n_clusters=5, linkage='ward', compute_full_tree=True).fit_predict(X)
    assert got.dtype == np.int64 and np.array_equal(got, want)


def test_refusals_happen_before_any_launch():
    from tvae import _lib, cluster
    from tvae._lib import TvaeHipError
    launches = []

    def hook(name, sig, args, do_call):
        launches.append(name)
        return do_call(args)

    old = _lib.set_call_hook(hook)
    try:
        with pytest.raises(TvaeHipError):
            cluster.ward_linkage(torch.zeros(8, 2))
        X = torch.randn(50, 3, device=DEV)
        X[17, 1] = float('nan')
        with pytest.raises(TvaeHipError, match='NaN or Inf'):
            cluster.ward_linkage(X)
        X[17, 1] = float('inf')
        with pytest.raises(TvaeHipError, match='NaN or Inf'):
            cluster.ward_linkage(X)
        with pytest.raises(TvaeHipError):
            cluster.ward_linkage(torch.randn(1, 3, device=DEV))
        with pytest.raises(TvaeHipError):
            cluster.ward_linkage(torch.randn(9, 257, device=DEV))
        assert launches == []
        X[17, 1] = 0.5
        cluster.ward_linkage(X)
        assert set(launches) == {'tvae_ward_nn', 'tvae_ward_merge'} and len(launches) % 2 == 0
    finally:
        _lib.set_call_hook(old)


def test_ward_host_switch_gives_the_same_clusters(tmp_path):
    """clustering_particles.py on tests/golden/stack_ref.mrcs with its default --clustering (agglomerative): the GPU path
    and TVAE_WARD=host (the reference's sklearn path) write the same clusters.npy."""
    pytest.importorskip('sklearn.cluster')
    import src.models as M
    torch.manual_seed(2)
    enc = M.InferenceNetwork_UnimodalTranslation_UnimodalRotation(36, 2 + 3, 16, num_layers=2)
    torch.save(enc, tmp_path / 'inference.sav')
    out = {}
    for mode in ('gpu', 'host'):
        cmd = [sys.executable, os.path.join(PKG, 'clustering_particles.py'), '--test-path',
               os.path.join(GOLDEN, 'stack_ref.mrcs'), '--crop', '6', '--t-inf', 'unimodal', '--r-inf', 'unimodal',
               '--n-clusters', '2', '--path-to-encoder', str(tmp_path / 'inference.sav'), '--out-dir', str(tmp_path / mode)]
        env = dict(os.environ)
        env.pop('TVAE_WARD', None)
        if mode == 'host':
            env['TVAE_WARD'] = 'host'
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert ('# ward linkage on the GPU' in r.stderr) == (mode == 'gpu')
        out[mode] = np.load(tmp_path / mode / 'clusters.npy')
    assert out['gpu'].shape == (5,) and sorted(set(out['gpu'].tolist())) == [0, 1]
    assert np.array_equal(out['gpu'], out['host'])
    assert np.array_equal(np.load(tmp_path / 'gpu' / 'latents.npy'), np.load(tmp_path / 'host' / 'latents.npy'))
