"""Host side of Ward clustering: ward_cut against sklearn's numbering on scipy's own linkage matrix, the C ABI of the
Ward entry points against the binding, and the argument checks (no GPU needed)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

CUT_INPUTS = [(300, 4, 1), (257, 2, 0), (130, 50, 3)]


def _points(N, d, seed):
    return np.random.default_rng(seed).standard_normal((N, d)).astype(np.float32)


def same_partition(a, b):
    a, b = np.asarray(a).tolist(), np.asarray(b).tolist()
    return len(set(zip(a, b))) == len(set(a)) == len(set(b))


@pytest.mark.parametrize('N,d,seed', CUT_INPUTS)
def test_ward_cut_numbers_clusters_as_sklearn(N, d, seed):
    sk = pytest.importorskip('sklearn.cluster')
    from scipy.cluster.hierarchy import ward
    from tvae import cluster
    X = _points(N, d, seed)
    Z = ward(X.astype(np.float64))
    for k in (1, 2, 5, 10, N):
        want = sk.AgglomerativeClustering(n_clusters=k, linkage='ward', compute_full_tree=True).fit_predict(X)
        got = cluster.ward_cut(Z, k)
        assert got.dtype == np.int64 and got.shape == (N,)
        assert np.array_equal(got, want), k


@pytest.mark.parametrize('N,d,seed', CUT_INPUTS)
def test_ward_cut_partition_is_the_maxclust_partition(N, d, seed):
    """Without sklearn: cutting the last k - 1 merges gives the partition of scipy's fcluster(maxclust) (heights are distinct
    here)."""
    from scipy.cluster.hierarchy import fcluster, ward
    from tvae import cluster
    Z = ward(_points(N, d, seed).astype(np.float64))
    for k in (1, 2, 5, 10, N):
        got = cluster.ward_cut(Z, k)
        assert sorted(set(got.tolist())) == list(range(k))
        assert same_partition(got, fcluster(Z, k, 'maxclust')), k


def test_ward_cut_on_a_chain_and_its_range_checks():
    """A dendrogram of depth N - 1 (every merge adds one leaf): the labels still reach the leaves."""
    from tvae import cluster
    N = 4000
    Z = np.zeros((N - 1, 4))
    Z[0, :2] = (0, 1)
    Z[1:, 0] = np.arange(2, N)
    Z[1:, 1] = N + np.arange(N - 2)
    Z[:, 2] = 1 + np.arange(N - 1)
    Z[:, 3] = 2 + np.arange(N - 1)
    lab = cluster.ward_cut(Z, 3)                      # the last two leaves alone, everything else together
    assert sorted(np.bincount(lab).tolist()) == [1, 1, N - 2]
    assert lab[N - 1] != lab[N - 2] and lab[N - 1] != lab[0] and lab[N - 2] != lab[0] and (lab[:N - 2] == lab[0]).all()
    assert np.array_equal(np.sort(cluster.ward_cut(Z, N)), np.arange(N))
    for bad in (0, N + 1):
        with pytest.raises(ValueError):
            cluster.ward_cut(Z, bad)
    with pytest.raises(ValueError):
        cluster.ward_cut(np.zeros((5, 3)), 2)


def test_ward_header_binding_and_queries():
    """The Ward names are declared in the header, bound, exported by the library, and the ABI version did not move."""
    from tvae import _cluster_lib as CL, _lib
    ward_calls = {'tvae_ward_nn', 'tvae_ward_merge'}
    ward_queries = {'tvae_ward_nn_ws_floats', 'tvae_ward_nn_splits', 'tvae_ward_merge_ws_ints'}
    assert ward_calls <= set(CL.SIGNATURES) and ward_queries <= set(CL.QUERIES)
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
    for name in ward_calls | ward_queries:
        assert re.search(r'\b(?:int|long)\s+' + name + r'\s*\(', hdr), name
    for name in ward_calls:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[-1].startswith('tvae_stream_t') and len(args) - 1 == len(CL.SIGNATURES[name])
        for pos, (a, c) in enumerate(zip(args, CL.SIGNATURES[name])):
            assert ('double*' in a) == ((name, pos) in _lib._F64_OK), (name, pos, a)
    L = CL.lib()
    for name in ward_calls | ward_queries:
        assert hasattr(L, name)
    assert L.tvae_cluster_abi_version() == CL.ABI_VERSION == 1
    # the column split depends on (M, d) only and the workspace is two words per (range, row)
    for M, d in [(2, 1), (65, 1), (257, 2), (4099, 4), (1000, 100), (40, 256), (100000, 100), (1 << 24, 4)]:
        S = CL.query('tvae_ward_nn_splits', M, d)
        assert 1 <= S <= 2048
        assert CL.query('tvae_ward_nn_ws_floats', M, d) == 2 * S * M
        assert CL.query('tvae_ward_merge_ws_ints', M, d) == 2 * M
    for bad in [(1, 4), (0, 4), ((1 << 24) + 1, 4), (100, 0), (100, 257)]:
        for q in sorted(ward_queries):
            assert CL.query(q, *bad) == 0, (q, bad)


def test_ward_linkage_argument_checks():
    from tvae import cluster
    from tvae._lib import TvaeHipError
    with pytest.raises(TvaeHipError, match='CUDA fp32'):
        cluster.ward_linkage(torch.zeros(8, 2))
    with pytest.raises(TvaeHipError, match='CUDA fp32'):
        cluster.ward_linkage(np.zeros((8, 2), np.float32))
    x = torch.zeros(8, 2)
    cluster._check_finite(x)
    for bad in (float('nan'), float('inf'), -float('inf')):
        y = x.clone()
        y[3, 1] = bad
        with pytest.raises(TvaeHipError, match='NaN or Inf'):
            cluster._check_finite(y)
    assert cluster.WARD_MAX_POINTS == 1 << 24


def test_agglomerative_keeps_the_host_path_for_host_arrays():
    """A numpy array or a CPU tensor goes to sklearn as before."""
    sk = pytest.importorskip('sklearn.cluster')
    from tvae import cluster
    X = _points(60, 3, 5)
    want = sk.AgglomerativeClustering(n_clusters=4, linkage='ward', compute_full_tree=True).fit_predict(X)
    assert np.array_equal(cluster.agglomerative(X, 4), want)
    assert np.array_equal(cluster.agglomerative(torch.from_numpy(X), 4), want)
