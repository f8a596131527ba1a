"""Host side of the t-SNE and the figures: the bisection and the symmetrisation of tvae.tsne on CPU tensors against sklearn's
own routines, the figures of tvae.figures from arrays alone, the header / binding of the t-SNE entry points and the
parsers of the four clustering scripts (no GPU needed).

Tolerances.  Entropy: the bisection stops within 1e-5 of ln(perplexity) and the returned row is fp32, which moves H by
up to K 2^-24 H ~ 1.9e-5 at K = 91; 2e-5 in all (the measured values are printed).  Against sklearn: two correct
searches may stop at opposite ends of the entropy window; 1e-4 of the row's (matrix's) largest entry."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

SHAPES = [(600, 4), (257, 2), (120, 4)]
PERPLEXITY = 30.0


def blobs(N, d, seed=0, centres=6, scale=6.0):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((centres, d)) * scale
    lab = np.arange(N) % centres
    return (C[lab] + rng.standard_normal((N, d))).astype(np.float32), lab


def knn_numpy(X, K):
    """(idx [N][K], squared distances fp32 [N][K]) by brute force in fp64, rows ascending by (distance, index)."""
    X64 = X.astype(np.float64)
    D = ((X64[:, None, :] - X64[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(D, np.inf)
    idx = np.argsort(D, axis=1, kind='stable')[:, :K]
    return idx.astype(np.int32), np.take_along_axis(D, idx, 1).astype(np.float32)


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def graph(request):
    """(N, K, idx, d2, conditional P of tvae.tsne on CPU tensors): computed once per shape, never modified."""
    from tvae import tsne
    N, d = request.param
    K = tsne.n_neighbors(N, PERPLEXITY)
    assert K == min(N - 1, 91)
    idx, d2 = knn_numpy(blobs(N, d, seed=N)[0], K)
    P = tsne.conditional_probabilities(torch.from_numpy(d2), PERPLEXITY)
    assert P.dtype == torch.float32 and not P.is_cuda and tuple(P.shape) == (N, K)
    return N, K, idx, d2, P.numpy()


def test_conditional_probabilities_rows(graph):
    N, K, idx, d2, P = graph
    P64 = P.astype(np.float64)
    assert (P >= 0).all()
    rowsum = np.abs(P64.sum(1) - 1).max()
    H = -(P64 * np.log(np.maximum(P64, 1e-300))).sum(1)
    herr = np.abs(H - np.log(PERPLEXITY)).max()
    print(f'conditional P {(N, K)}: |row sum - 1| <= {rowsum:.3e}, |H - ln 30| <= {herr:.3e}')
    assert rowsum <= 1e-6
    assert herr <= 2e-5


def test_conditional_probabilities_against_sklearn(graph):
    utils = pytest.importorskip('sklearn.manifold._utils')
    N, K, idx, d2, P = graph
    want = utils._binary_search_perplexity(np.ascontiguousarray(d2), PERPLEXITY, 0)
    err = (np.abs(P - want).max(1) / want.max(1)).max()
    print(f'conditional P {(N, K)} against sklearn: {err:.3e} of the row maximum')
    assert err <= 1e-4


def test_joint_probabilities(graph):
    from tvae import tsne
    N, K, idx, d2, P = graph
    csr = tsne.joint_probabilities(torch.from_numpy(idx), torch.from_numpy(P))
    rowptr, col, val = csr.rowptr.numpy(), csr.col.numpy(), csr.val.numpy()
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32
    assert rowptr.shape == (N + 1,) and rowptr[0] == 0 and rowptr[-1] == col.size == val.size
    assert (np.diff(rowptr) >= K).all() and N * K <= col.size <= 2 * N * K
    assert ((col >= 0) & (col < N)).all()
    dense = np.zeros((N, N), np.float32)
    for i in range(N):
        c = col[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(c) > 0).all() and i not in c               # ascending, no diagonal
        dense[i, c] = val[rowptr[i]:rowptr[i + 1]]
    assert np.array_equal(dense, dense.T)                           # exactly symmetric
    assert abs(float(dense.astype(np.float64).sum()) - 1) <= 1e-5
    tsne_sk = pytest.importorskip('sklearn.manifold._t_sne')
    from scipy.sparse import csr_matrix
    order = np.argsort(idx, axis=1)                                 # sklearn wants sorted indices; same graph
    Dn = csr_matrix((np.take_along_axis(d2, order, 1).ravel(), np.take_along_axis(idx, order, 1).ravel(),
                     np.arange(0, N * K + 1, K)), shape=(N, N))
    want = tsne_sk._joint_probabilities_nn(Dn, PERPLEXITY, 0).toarray()
    err = np.abs(dense - want).max() / want.max()
    print(f'joint P {(N, K)} against sklearn: {err:.3e} of the maximum')
    assert err <= 1e-4


def test_joint_probabilities_refuses_indices_outside_the_points(graph):
    """tvae_knn leaves -1 where a row has fewer than K finite distances; such an index must not reach the row * N + col keys."""
    from tvae import tsne
    from tvae._lib import TvaeHipError
    N, K, idx, d2, P = graph
    for bad in (-1, N):
        broken = idx.copy()
        broken[N // 2, K - 1] = bad
        with pytest.raises(TvaeHipError, match='outside'):
            tsne.joint_probabilities(torch.from_numpy(broken), torch.from_numpy(P))


def test_figures_from_arrays(tmp_path):
    pytest.importorskip('matplotlib')
    from PIL import Image
    from tvae import cluster, figures
    rng = np.random.default_rng(0)
    N = 60
    labels = np.arange(N) % 3
    clusters = (labels + 1) % 3
    clusters[:5] = labels[:5]
    emb = rng.standard_normal((N, 2)) + 4 * labels[:, None]
    mapping, _ = cluster.cluster_acc(labels, clusters)
    out = str(tmp_path)
    paths = [figures.save_tsne(out, emb, labels),
             figures.save_confusion_matrix(out, labels, clusters, mapping[1]),
             figures.save_z_vals(out, rng.standard_normal((N, 4)), clusters)]
    paths += figures.save_histograms(out, rng.uniform(-3, 3, (N, 1)), rng.standard_normal((N, 2)))
    names = ['tsne.jpg', 'confusion_matrix.jpg', 'z_vals.jpg', 'predicted_rotation_vals.jpg',
             'predicted_translation_x_vals.jpg', 'predicted_translation_y_vals.jpg']
    assert [os.path.basename(p) for p in paths] == names
    for name in names:
        with Image.open(os.path.join(out, name)) as im:
            assert im.format == 'JPEG' and min(im.size) >= 500, (name, im.size)
            assert np.asarray(im.convert('L')).std() > 1, name      # not a blank canvas
    # the confusion matrix itself, and its columns under the cluster_acc mapping: the diagonal holds the matched counts
    cm = figures.confusion_counts(labels, clusters)
    assert cm.sum() == N and cm[0, 0] == 2 and cm[0, 1] == 18
    assert np.trace(cm[:, np.asarray(mapping[1])]) == 55
    figures.save_tsne(out, emb, None)                               # a stack without labels


def test_parsers_still_have_exactly_todays_flags():
    from tvae import cluster_driver
    ref = json.load(open(os.path.join(GOLDEN, 'cli_flags_clustering.json')))
    for script, flags in ref.items():
        parser = cluster_driver.build_parser(script.replace('clustering_', ''))
        mine = {a.dest for a in parser._actions if a.dest != 'help'}
        assert mine == set(flags) | {'seed', 'n_init', 'out_dir'}, script


def test_tsne_header_binding_and_queries():
    from tvae import _cluster_lib as CL, _lib
    calls = {'tvae_knn', 'tvae_tsne_repulsion', 'tvae_tsne_step', 'tvae_tsne_kl'}
    queries = {'tvae_tsne_groups', 'tvae_tsne_repulsion_ws_floats'}
    assert calls <= set(CL.SIGNATURES) and queries <= set(CL.QUERIES)
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
    for name in calls:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[-1].startswith('tvae_stream_t') and len(args) - 1 == len(CL.SIGNATURES[name])
        for pos, (a, c) in enumerate(zip(args, CL.SIGNATURES[name])):
            assert ('double*' in a) == ((name, pos) in _lib._F64_OK), (name, pos, a)
    L = CL.lib()
    for name in calls | queries:
        assert hasattr(L, name), name
    assert L.tvae_cluster_abi_version() == CL.ABI_VERSION == 1
    for N in (2, 257, 1000, 4099, 10000, 737280, 1 << 24):
        G = CL.query('tvae_tsne_groups', N)
        assert G == (N + 255) // 256
        ws = CL.query('tvae_tsne_repulsion_ws_floats', N)
        S = (ws - 2 * G) // (3 * N)
        assert ws == 2 * G + 3 * S * N and 1 <= S <= 2048 and G * S <= max(2048, G)
    for bad in (1, 0, -5, (1 << 24) + 1):
        assert CL.query('tvae_tsne_groups', bad) == 0 and CL.query('tvae_tsne_repulsion_ws_floats', bad) == 0


def test_tsne_argument_checks():
    from tvae import tsne
    from tvae._lib import TvaeHipError
    with pytest.raises(TvaeHipError, match='CUDA fp32'):
        tsne.tsne(torch.zeros(100, 4))
    with pytest.raises(TvaeHipError, match='CUDA fp32'):
        tsne.knn(np.zeros((100, 4), np.float32), 5)
    with pytest.raises(TvaeHipError):
        tsne.gradient(torch.zeros(8, 2), None)
