"""Eigenimages of the aligned classes, the part that needs no GPU: the header against the binding for the new names, the
workspace queries, tests/eigen_ref.py against itself (backproject(project(V)) against the explicit R^T R V, its subspace
iteration against numpy's SVD on the planted case), the conditions on the planted case that the GPU tests lean on,
tvae.eigen.orthonormalise on CPU tensors, the argument checks and the parsers.

The planted case (eigen_ref.planted): smooth Hermite functions, three planted components with sigma halving, J = 4, rendered
into every particle's frame in fp64.  Conditions checked here on the reference and the bounds alone:
  * truncation: (lambda_{J+1} / lambda_j)^(2 passes) <= 1e-8 for the three compared components;
  * the sine bound 2 dS / ((m - 1) gap_j) <= 3e-2 for the three;
  * the eigenvalue tolerance 2 dS / (m - 1) <= 1e-3 lambda_j.
All three hold, the last one narrowly for component 2 (tolerance / lambda = 9.7e-4 at both geometries): with sigma halving
the tolerance is about 4 |B|_F / |R|_F of the TOTAL variance, and |B|_F / |R|_F cannot go much below 1e-5 with the sampling
bound of test_align_gpu.image_bounds (delta = 16 2^-24 (2 + t |dx|) (n - 1) / 2 pixels times twice the steepest step of an
image whose content must be small at the frame's edge).  The shapes of eigen_ref.planted_modes are the best of a scan over
Hermite orders up to 3 and widths of 0.2 .. 0.3 of the half side, in the natural normalisation, which gives the higher orders
more weight and keeps the third eigenvalue at about a third of the first; every channel carries the full amplitude.
"""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import align_ref
import eigen_ref as ER
import test_align_gpu as TA
from conftest import PKG, ROOT

# ---- header, binding, queries ----------------------------------------------------------------------------------------------
NEW_CALLS = {'tvae_class_project': 'ppppp' 'pp' 'pp' 'p' 'l' 'iiiii' 'fff',
             'tvae_class_backproject': 'ppppp' 'pp' 'pp' 'p' 'l' 'iiiii' 'fff'}
NEW_QUERIES = {'tvae_class_project_ws_floats': ('iiiii', 'l'), 'tvae_class_backproject_ws_floats': ('iiiii', 'l'),
               'tvae_class_eigen_chunk': ('iiiii', 'i')}


def test_header_and_binding_of_the_new_entry_points():
    from tvae import _cluster_lib as CL
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
    assert re.search(r'#define\s+TVAE_EIGEN_MAX_COMPONENTS\s+16\b', hdr)
    for name, sig in NEW_CALLS.items():
        assert CL.SIGNATURES[name] == sig
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[-1].startswith('tvae_stream_t') and len(args) - 1 == len(sig)
        for a, c in zip(args[:-1], sig):
            assert ('*' in a) == (c == 'p') and a.startswith({'p': ('const ', 'float', 'int'), 'f': 'float ', 'l': 'long ',
                                                               'i': 'int '}[c]), (name, a)
    for name, (sig, ret) in NEW_QUERIES.items():
        assert CL.QUERIES[name] == (sig, ret)
        m = re.search(r'\b(int|long)\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m and m.group(1) == {'l': 'long', 'i': 'int'}[ret] and len(m.group(2).split(',')) == len(sig), name
    assert CL.ABI_VERSION == 1 and re.search(r'tvae_cluster_abi_version\(void\);\s*/\* == 1 \*/', hdr)


def test_the_built_library_exports_the_new_symbols():
    from tvae import _cluster_lib as CL
    L = CL.lib()
    for name in list(NEW_CALLS) + list(NEW_QUERIES):
        assert getattr(L, name) is not None
    assert L.tvae_cluster_abi_version() == 1


def test_queries_return_the_documented_sizes_and_zero_for_bad_arguments():
    from tvae import _cluster_lib as CL
    from tvae import eigen
    for N, K, C, n, J in [(400, 5, 3, 33, 3), (100000, 10, 1, 128, 8), (20000, 10, 1, 128, 16), (1, 1, 1, 2, 1),
                          (7, 3, 2, 1024, 5)]:
        chunk = CL.query('tvae_class_eigen_chunk', N, K, C, n, J)
        assert chunk == eigen.chunk_members(N, K, C, n, J)
        assert chunk > CL.query('tvae_class_average_chunk', N, K, C, n) and 300 > 2 * chunk
        assert chunk == CL.query('tvae_class_eigen_chunk', N, K + 1, C, n, 1)       # a constant of the build
        slots = N // chunk + K
        assert CL.query('tvae_class_project_ws_floats', N, K, C, n, J) == (K + 1 + 3) // 4 * 4 + n * n
        assert CL.query('tvae_class_backproject_ws_floats', N, K, C, n, J) == \
            (K + 1 + slots + 3) // 4 * 4 + n * n + slots * J * C * n * n
    # what the header states for 100 000 x 128 x 128, K = 10, J = 8: 791 slots of 512 KB
    assert 100000 // CL.query('tvae_class_eigen_chunk', 100000, 10, 1, 128, 8) + 10 == 791
    assert round(CL.query('tvae_class_backproject_ws_floats', 100000, 10, 1, 128, 8) * 4 / 1e6) == 415
    for bad in [(400, 5, 1, 1, 3), (400, 5, 1, 1025, 3), (400, 0, 1, 16, 3), (400, 5, 0, 16, 3), (0, 5, 1, 16, 3),
                (-1, 5, 1, 16, 3), (400, 65536, 1, 16, 3), (400, 5, 1025, 16, 3), ((1 << 24) + 1, 5, 1, 16, 3),
                (400, 5, 1, 16, 0), (400, 5, 1, 16, 17), (400, 5, 1, 16, -1), (1 << 24, 5, 64, 1024, 3),
                (400, 65535, 1024, 1024, 16)]:
        for q in NEW_QUERIES:
            assert CL.query(q, *bad) == 0, (q, bad)


# ---- the restatement against itself -------------------------------------------------------------------------------------------
def test_restatement_backproject_of_project_is_the_explicit_gram_product():
    rng = np.random.default_rng(5)
    N, K, C, n, J = 40, 3, 2, 7, 3
    Y = rng.standard_normal((N, C, n, n))
    theta, dx = rng.uniform(-3, 3, N), rng.uniform(-0.3, 0.3, (N, 2))
    A = align_ref.align_stack(Y, theta, dx, 1.0)
    labels = rng.integers(0, K, N)
    order, seg, counts = align_ref.segments(labels, K)
    order = order.copy()
    order[[3, 17]] = [-1, N]                                             # two skipped entries
    mean = rng.standard_normal((K, C, n, n))
    V = rng.standard_normal((K, J, C, n, n))
    mk = ER.mask(n, 2.0, 1.5)
    assert mk.max() == 1.0 and mk.min() == 0.0 and ((mk > 0) & (mk < 1)).any()
    assert np.array_equal(ER.mask(n, 0.0, 1.0), np.ones((n, n))) and np.array_equal(ER.mask(n, None), np.ones((n, n)))
    hard = ER.mask(n, 2.0, 0.0)
    assert set(np.unique(hard)) == {0.0, 1.0}
    coef, norm2 = ER.project(A, mean, V, order, seg, mk)
    W, cnt = ER.backproject(A, mean, coef, order, seg, mk)
    assert not coef[[3, 17]].any() and not norm2[[3, 17]].any()
    assert cnt.sum() == N - 2
    for k in range(K):
        q, ids = ER.members(order, seg, k, N)
        R = np.stack([(mk[None] * (A[i] - mean[k])).reshape(-1) for i in ids])
        want = (R.T @ R @ V[k].reshape(J, -1).T).T
        assert np.allclose(W[k].reshape(J, -1), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        assert np.allclose(norm2[q], (R * R).sum(1), rtol=1e-13)


@pytest.fixture(scope='module', params=[(33, 1), (16, 3)], ids=['33x1', '16x3'])
def planted(request):
    return ER.planted_reference(*request.param, TA.image_bounds)


def test_restatement_subspace_iteration_agrees_with_the_svd_on_the_planted_case(planted):
    c = planted
    J, L = ER.PLANTED_J, ER.PLANTED_J + 4
    V0 = np.random.default_rng(1).standard_normal((L, c['R'].shape[1]))
    lam, vec, y = ER.subspace_iteration(c['R'], J, 4, ER.PLANTED_PASSES - 1, V0)
    for j in range(3):
        cos = abs(vec[j] @ c['vec'][j])
        print(f'component {j}: lambda {lam[j]:.6e} against {c["lam"][j]:.6e}, 1 - |cos| = {1 - cos:.2e}')
        assert abs(lam[j] - c['lam'][j]) <= 1e-9 * c['lam'][j] and 1 - cos <= 1e-9
        s = np.sign(vec[j] @ c['vec'][j])
        assert np.abs(y[:, j] * s - c['coords'][:, j]).max() <= 1e-6 * np.abs(c['coords'][:, j]).max()
    assert np.allclose(vec @ vec.T, np.eye(J), atol=1e-12)


def test_restatement_rank_deficiency_gives_exact_zeros():
    rng = np.random.default_rng(2)
    R = rng.standard_normal((3, 50))
    R -= R.mean(0)                                                       # rank 2
    lam, vec, y = ER.subspace_iteration(R, 4, 4, 2, rng.standard_normal((8, 50)))
    assert (lam[:2] > 0).all() and not lam[2:].any() and not vec[2:].any() and not y[:, 2:].any()
    assert np.allclose(lam[:2], ER.svd_reference(R)[0][:2], rtol=1e-10)


def test_planted_truncation_and_sine_caps(planted):
    c = planted
    lam = c['lam']
    assert np.all(np.diff(lam[:4]) < 0)
    for j in range(3):
        trunc = (lam[ER.PLANTED_J] / lam[j]) ** (2 * ER.PLANTED_PASSES)
        print(f'component {j}: lambda {lam[j]:.4e}, gap {c["gap"][j]:.4e}, truncation {trunc:.1e}, sine bound {c["sine"][j]:.2e}')
        assert trunc <= 1e-8
        assert c['sine'][j] <= 3e-2
    # sigma halving: the planted amplitudes are what they are said to be, and the fourth direction is noise
    assert ER.PLANTED_SIGMA == (1.0, 0.5, 0.25) and lam[3] < 1e-3 * lam[2]


@pytest.mark.parametrize('j', [0, 1, 2])
def test_planted_eigenvalue_cap(planted, j):
    """lam_tol <= 1e-3 lambda_j for every compared component."""
    c = planted
    print(f'component {j}: tolerance / lambda = {c["lam_tol"] / c["lam"][j]:.3e}')
    assert c['lam_tol'] <= 1e-3 * c['lam'][j]


# ---- tvae.eigen on the host ----------------------------------------------------------------------------------------------------
def test_orthonormalise_on_cpu_tensors():
    from tvae import eigen
    rng = np.random.default_rng(3)
    W = rng.standard_normal((3, 6, 40))
    W[1, 4] = W[1, 0] + W[1, 1]                                          # rows 0, 1, 2 span class 1: rank 3
    W[1, 5] = 0.0
    W[1, 3] = 2 * W[1, 2]
    W[2] = 0.0
    Q, rank = eigen.orthonormalise(torch.from_numpy(W.astype(np.float32)))
    Q = Q.numpy()
    assert Q.dtype == np.float64 and rank.tolist() == [6, 3, 0]
    assert np.allclose(Q[0] @ Q[0].T, np.eye(6), atol=1e-12)
    assert np.allclose(Q[1, :3] @ Q[1, :3].T, np.eye(3), atol=1e-12) and not Q[1, 3:].any() and not Q[2].any()
    Wf = W.astype(np.float32).astype(np.float64)
    proj = Q[1, :3].T @ (Q[1, :3] @ Wf[1].T)                             # the rows of W lie in the span of Q
    assert np.allclose(proj, Wf[1].T, atol=1e-6)
    ref, r = ER.orthonormalise(Wf[1])
    assert r == 3 and not ref[3:].any() and np.allclose(ref[:3].T @ ref[:3], Q[1, :3].T @ Q[1, :3], atol=1e-6)
    bad = torch.from_numpy(W.astype(np.float32))
    bad[0, 0, 0] = float('nan')
    Q, rank = eigen.orthonormalise(bad)
    assert rank.tolist() == [0, 3, 0] and not Q[0].any()


def test_cpu_tensors_and_bad_arguments_are_refused():
    from tvae import eigen
    y, th, dx = torch.zeros(4, 1, 8, 8), torch.zeros(4), torch.zeros(4, 2)
    order, seg = torch.arange(4, dtype=torch.int32), torch.tensor([0, 2, 4], dtype=torch.int32)
    mean, V, coef = torch.zeros(2, 1, 8, 8), torch.zeros(2, 3, 1, 8, 8), torch.zeros(4, 3)
    with pytest.raises(eigen.TvaeHipError):
        eigen.project(y, th, dx, order, seg, mean, V)
    with pytest.raises(eigen.TvaeHipError):
        eigen.backproject(y, th, dx, order, seg, mean, coef)
    with pytest.raises(eigen.TvaeHipError):
        eigen.class_eigenimages(y, th, dx, torch.zeros(4, dtype=torch.int64), 2)
    for r, e in [(float('nan'), 1.0), (2.0, float('inf')), (2.0, -1.0)]:
        with pytest.raises(eigen.TvaeHipError):
            eigen._mask(r, e, 'project')
    assert eigen._mask(None, 0.0, 'project') == (0.0, 0.0) and eigen.MAX_COMPONENTS == 16


# ---- parsers ---------------------------------------------------------------------------------------------------------------
def _flags(parser):
    return sorted(s for a in parser._actions for s in a.option_strings if s not in ('-h', '--help'))


def test_class_eigenimages_parser():
    from tvae import eigen, resolution
    base = ['--stack', '--rotations', '--translations', '--clusters', '--t-inf', '--crop', '--n-clusters', '--out-dir',
            '--mask-radius', '--mask-edge', '-d', '--device', '--components', '--oversample', '--power-iterations', '--seed']
    assert _flags(eigen.build_parser()) == sorted(base)
    assert _flags(eigen.build_parser(ctf=True)) == sorted(base + ['--ctf', '--ctf-correct', '--scale'])
    # every flag of class_resolution.py but the two that belong to the FRC
    assert set(_flags(resolution.build_parser(ctf=True))) - set(_flags(eigen.build_parser(ctf=True))) == {'--apix', '--threshold'}
    need = ['--stack', 's.mrcs', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy']
    a = eigen.build_parser(ctf=True).parse_args(need)
    assert (a.components, a.oversample, a.power_iterations, a.seed, a.mask_radius, a.mask_edge, a.ctf, a.ctf_correct) == \
        (4, 4, 2, 0, None, resolution.MASK_EDGE, None, 'flip')
    a = eigen.build_parser(ctf=True).parse_args(need + ['--components', '8', '--oversample', '2', '--power-iterations', '1',
                                                        '--seed', '5', '--ctf', 'c.txt', '--t-inf', 'unimodal'])
    assert (a.components, a.oversample, a.power_iterations, a.seed, a.ctf, a.t_inf) == (8, 2, 1, 5, 'c.txt', 'unimodal')
    with pytest.raises(SystemExit):
        eigen.build_parser(ctf=True).parse_args(need + ['--ctf-correct', 'wiener'])
    spec = importlib.util.spec_from_file_location('class_eigenimages_script', os.path.join(PKG, 'class_eigenimages.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run is eigen.run and callable(mod.main)


def test_eigen_bench_parser():
    spec = importlib.util.spec_from_file_location('eigen_bench', os.path.join(ROOT, 'profiles', 'tools', 'eigen_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert _flags(p) == sorted(['--shapes', '--clusters', '--components', '--reps', '--warmup', '--out', '--tag'])
    a = p.parse_args([])
    assert a.shapes == ['100000x64', '20000x128'] and a.clusters == 10 and a.components == [4, 8]
    assert (a.reps, a.warmup) == (10, 2) and mod.parse_shape('20000x128') == (20000, 128)


def test_the_clustering_parsers_gained_no_flag():
    from tvae import cluster_driver
    flags = _flags(cluster_driver.build_parser('particles'))
    assert not [f for f in flags if 'eigen' in f or 'component' in f]
