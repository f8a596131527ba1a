"""Maximum-likelihood class averages, the part that needs no GPU: the header against the binding and the built library for the
new names, the workspace queries, tests/ml_ref.py against itself and against align_ref, tvae.ml2d.entries_by_class on CPU
tensors against a Python loop, the sigma^2 / prior / log-likelihood helpers against fp64, the parser of
ml_class_averages.py, and the condition on the reference's own top-P sets that the GPU test of the loop leans on."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import align_ref
import ml_ref
import pose_ref
from conftest import PKG, ROOT
from tvae import ml2d        # at module level: every test of this file needs the feature, the reference's own among them

F32 = np.float32

# ---- header, binding, queries ----------------------------------------------------------------------------------------------
NEW_CALLS = {'tvae_pose_posterior': 'ppppp' 'pp' 'ppppp' 'pppp' 'iiiiiii' 'fff',
             'tvae_class_average_weighted': 'pppppp' 'pppp' 'l' 'iiiii' 'f'}
NEW_QUERIES = {'tvae_class_average_weighted_ws_floats': ('iiii', 'l'), 'tvae_class_average_weighted_chunk': ('iiii', 'i')}
F64_ARGS = {('tvae_pose_posterior', 4), ('tvae_pose_posterior', 13), ('tvae_pose_posterior', 14), ('tvae_class_average_weighted', 7)}


def test_header_binding_and_library_agree_on_the_new_entry_points():
    from tvae import _cluster_lib as CL, _lib
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
    for name, sig in NEW_CALLS.items():
        assert CL.SIGNATURES[name] == sig
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[-1].startswith('tvae_stream_t') and len(args) - 1 == len(sig)
        for pos, (a, c) in enumerate(zip(args[:-1], sig)):
            assert ('*' in a) == (c == 'p'), (name, a)
            if c == 'p':
                assert ('double*' in a) == ((name, pos) in F64_ARGS) == ((name, pos) in _lib._F64_OK), (name, pos, a)
            else:
                assert a.startswith({'f': 'float ', 'l': 'long ', 'i': 'int '}[c]), (name, a)
    for name, (sig, ret) in NEW_QUERIES.items():
        assert CL.QUERIES[name] == (sig, ret)
        m = re.search(r'\b(int|long)\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m and m.group(1) == {'i': 'int', 'l': 'long'}[ret]
        assert all(a.strip().startswith('int ') for a in m.group(2).split(',')) and len(m.group(2).split(',')) == len(sig)
    declared = set(re.findall(r'\b(?:int|long)\s+(tvae_\w+)\s*\(', hdr))
    assert {n for n in declared if 'posterior' in n or 'weighted' in n} == set(NEW_CALLS) | set(NEW_QUERIES)
    assert re.search(r'#define\s+TVAE_POSTERIOR_MAX_KEEP\s+64\b', hdr)
    L = CL.lib()
    assert L.tvae_cluster_abi_version() == 1
    for name in list(NEW_CALLS) + list(NEW_QUERIES):
        assert hasattr(L, name), name
    flat = ' '.join(hdr.split())
    assert 'l_j stays in LDS for J <= 4096' in flat and 'l descending, then j ascending' in flat and 'acc = fma(w_e, a_e, acc)' in flat and 'avg[k] = (float)(S / W_k)' in flat


def test_queries():
    from tvae import _cluster_lib as CL
    from tvae import ml2d
    for E, K, C, n in [(1, 1, 1, 2), (800, 10, 1, 64), (127, 3, 2, 17), (128, 3, 2, 17), (1 << 20, 10, 1, 128), (1 << 30, 1, 1, 2)]:
        chunk = CL.query('tvae_class_average_weighted_chunk', E, K, C, n)
        assert chunk == 128 == ml2d.chunk_entries(E, K, C, n)
        slots = E // chunk + K
        ints = (K + 1 + slots + 3) // 4 * 4
        assert CL.query('tvae_class_average_weighted_ws_floats', E, K, C, n) == ints + 2 * slots + slots * C * n * n
    for bad in [(0, 2, 1, 8), ((1 << 30) + 1, 2, 1, 8), (-4, 2, 1, 8), (8, 0, 1, 8), (8, 65536, 1, 8), (8, 2, 0, 8), (8, 2, 1025, 8),
                (8, 2, 1, 1), (8, 2, 1, 1025), (1 << 30, 1, 1, 1024)]:
        assert CL.query('tvae_class_average_weighted_ws_floats', *bad) == 0, bad
        assert CL.query('tvae_class_average_weighted_chunk', *bad) == 0, bad


# ---- the reference against itself ------------------------------------------------------------------------------------------------
def random_tables(rng, N, M, A, S, K):
    NA, NS = 2 * A + 1, 2 * S + 1
    pp = rng.uniform(50, 150, (N, M, NA, NS, NS)).astype(F32)
    yy = rng.uniform(100, 200, N).astype(F32)
    num = rng.uniform(-40, 90, (N, M, NA, NS, NS)).astype(F32)
    cand = np.stack([rng.permutation(K)[:M] for _ in range(N)])
    return num, pp, yy, cand


def test_reference_weights_sum_to_one():
    rng = np.random.default_rng(0)
    N, M, A, S, K, P, n = 7, 3, 2, 1, 5, 6, 16
    num, pp, yy, cand = random_tables(rng, N, M, A, S, K)
    cand[1] = -1                                              # a dead image
    cand[2, 1] = K                                            # an invalid slot
    num[3, 0, 1, 1, 1] = np.nan
    lp = np.log(rng.dirichlet(np.ones(K)))
    theta, dx = rng.uniform(-3, 3, N).astype(F32), rng.uniform(-0.2, 0.2, (N, 2)).astype(F32)
    r = ml_ref.posterior(num, pp, yy, cand, lp, theta, dx, n, K, A, S, P, 1.0, 0.05, 30.0)
    live = r['live']
    assert live.tolist() == [True, False, True, True, True, True, True]
    assert np.allclose(r['resp'][live].sum(1), 1.0, rtol=0, atol=1e-14) and np.allclose(r['w'][live].sum(1), 1.0, rtol=0, atol=1e-14)
    assert not r['resp'][1].any() and not r['w'][1].any() and (r['idx'][1] == -1).all() and r['lse'][1] == 0 and r['kept'][1] == 0
    assert not r['resp'][2, 1] and np.isnan(r['l'][3].reshape(M, -1)[0, (1 * 3 + 1) * 3 + 1])
    assert (r['kept'][live] > 0).all() and (r['kept'] <= 1 + 1e-15).all()
    assert (np.diff(r['wj'][live], axis=1) <= 0).all()       # rank order
    # lse is the log of the summed likelihoods, whatever L is
    l = r['l'][0][~np.isnan(r['l'][0])]
    assert abs(r['lse'][0] - math.log(np.exp(l - l.mean()).sum()) - l.mean()) <= 1e-12 * abs(r['lse'][0])
    # the pose of a kept candidate is pose_ref.update_pose of its indices; an empty rank keeps the image's pose bit for bit
    NS, cnd = 2 * S + 1, (2 * A + 1) * (2 * S + 1) ** 2
    j = r['idx'][0, 0]
    c = j % cnd
    th, d = pose_ref.update_pose(theta[:1], dx[:1], np.array([[c // (NS * NS) - A, (c // NS) % NS - S, c % NS - S]]), n, 1.0, 0.05)
    assert r['theta'][0, 0].tobytes() == th[0].tobytes() and r['dx'][0, 0].tobytes() == d[0].tobytes()
    assert r['theta'][1].tobytes() == np.repeat(theta[1], P).tobytes()
    # P beyond the live candidates: padding
    r = ml_ref.posterior(num[:, :1, 1:2], pp[:, :1, 1:2], yy, cand[:, :1], None, theta, dx, n, K, 0, S, 16, 1.0, 0.05, 30.0)
    assert (r['idx'][0, :9] >= 0).all() and (r['idx'][0, 9:] == -1).all() and not r['w'][0, 9:].any()
    assert (r['idx'][3, :8] >= 0).all() and (r['idx'][3, 8:] == -1).all()       # the NaN entry is out


def test_reference_weighted_average_with_unit_weights_is_the_class_average():
    rng = np.random.default_rng(1)
    N, C, n, K = 30, 2, 9, 4
    Y = rng.standard_normal((N, C, n, n)).astype(F32)
    theta, dx = rng.uniform(-3, 3, N).astype(F32), rng.uniform(-0.3, 0.3, (N, 2)).astype(F32)
    labels = rng.integers(0, K, N)
    labels[labels == 2] = 0                                   # an empty class
    order, seg, counts = align_ref.segments(labels, K)
    want, cnt = align_ref.class_averages(align_ref.align_stack(Y, theta, dx, 1.0), order, seg)
    got = ml_ref.weighted_averages(Y, order, theta[order], dx[order], np.ones(N, dtype=F32), seg, 1.0, 128)
    assert np.allclose(got['avg'], want, rtol=0, atol=1e-14) and got['counts'].tolist() == cnt.tolist() == counts.tolist()
    assert got['wsum'].tolist() == counts.astype(np.float64).tolist() and not got['avg'][2].any()
    # the weights scale out; dead entries count for nothing
    w = np.full(N, 0.25, dtype=F32)
    img = order.copy()
    dead = [0, 7, 11, 19]
    img[dead[0]], img[dead[1]] = -1, N
    w[dead[2]], w[dead[3]] = np.nan, -1.0
    got = ml_ref.weighted_averages(Y, img, theta[order], dx[order], w, seg, 1.0, 128)
    keep = np.ones(N, dtype=bool)
    keep[dead] = False
    lab2 = np.where(keep[np.argsort(order)], labels, -1)
    o2, s2, c2 = align_ref.segments(lab2, K)
    want2, _ = align_ref.class_averages(align_ref.align_stack(Y, theta, dx, 1.0), o2, s2)
    assert np.allclose(got['avg'], want2, rtol=0, atol=1e-14) and got['counts'].tolist() == c2.tolist()
    assert np.allclose(got['wsum'], 0.25 * c2, rtol=0, atol=1e-15)
    assert ml_ref.clean_seg([-7, 12, 10, -5, 39, 1000], 40).tolist() == [0, 12, 12, 12, 39, 40]


# ---- entries_by_class ----------------------------------------------------------------------------------------------------------
def test_entries_by_class_on_cpu_tensors():
    from tvae import ml2d
    rng = np.random.default_rng(2)
    N, P, K = 23, 5, 6
    cls = rng.integers(-1, K + 1, (N, P))
    cls[cls == 4] = 1                                         # an empty class; -1 and K are dropped
    w = rng.uniform(0, 1, (N, P)).astype(F32)
    th = rng.uniform(-3, 3, (N, P)).astype(F32)
    d = rng.uniform(-1, 1, (N, P, 2)).astype(F32)
    want = ml_ref.entries_by_class(cls, w, th, d, K)
    got = ml2d.entries_by_class(torch.from_numpy(cls), torch.from_numpy(w), torch.from_numpy(th), torch.from_numpy(d), K)
    assert got['img'].dtype == torch.int32 and got['seg'].dtype == torch.int32 and got['w'].dtype == torch.float32
    assert not got['img'].is_cuda
    for key in ('img', 'theta', 'dx', 'w', 'seg'):
        assert np.array_equal(got[key].numpy(), want[key]), key
    seg = got['seg'].numpy()
    assert seg[0] == 0 and seg[-1] == ((cls >= 0) & (cls < K)).sum() and seg[4] == seg[5] and (np.diff(seg) >= 0).all()
    for k in range(K):                                        # stable: ascending (image, rank) within a class
        img = got['img'].numpy()[seg[k]:seg[k + 1]]
        assert (np.diff(img) >= 0).all()
        ii, pp = np.nonzero(cls == k)
        assert np.array_equal(img, ii) and np.array_equal(got['w'].numpy()[seg[k]:seg[k + 1]], w[ii, pp])
    # int32 classes as the kernel writes them, and nothing left at all
    again = ml2d.entries_by_class(torch.from_numpy(cls.astype(np.int32)), w, th, d, K)
    assert all(torch.equal(again[key], got[key]) for key in got)
    none = ml2d.entries_by_class(np.full((3, 2), -1), np.zeros((3, 2), F32), np.zeros((3, 2), F32), np.zeros((3, 2, 2), F32), 2)
    assert none['img'].numel() == 0 and none['seg'].tolist() == [0, 0, 0] and tuple(none['dx'].shape) == (0, 2)
    from tvae._lib import TvaeHipError
    for bad in [(cls.astype(np.float32), w, th, d, K), (cls, w[:, :2], th, d, K), (cls, w, th, d[:, :, :1], K), (cls, w, th, d, 0)]:
        with pytest.raises(TvaeHipError):
            ml2d.entries_by_class(*bad)


# ---- the updates of a round --------------------------------------------------------------------------------------------------------
def test_update_helpers_against_fp64():
    from tvae import ml2d
    rng = np.random.default_rng(3)
    N, C, n, A, S = 40, 2, 17, 3, 2
    r2 = rng.uniform(500, 700, N)
    lse = rng.uniform(-900, -500, N)
    live = rng.uniform(size=N) > 0.2
    s2 = ml2d.update_sigma2(torch.from_numpy(r2), torch.from_numpy(live), C, n)
    assert s2 == pytest.approx(ml_ref.update_sigma2(r2, live, C, n), rel=1e-14)
    assert s2 == pytest.approx(r2[live].sum() / (live.sum() * C * n * n), rel=1e-14)
    assert math.isnan(ml2d.update_sigma2(r2, np.zeros(N, dtype=bool), C, n))
    wsum = np.array([3.5, 0.0, 1.25, 7.0])
    pi, lp = ml2d.update_priors(torch.from_numpy(wsum))
    rpi, rlp = ml_ref.update_priors(wsum)
    assert pi.dtype == torch.float64 and np.allclose(pi.numpy(), rpi, rtol=1e-15, atol=0) and pi.numpy().sum() == pytest.approx(1.0)
    assert lp[1] == -math.inf and np.allclose(lp.numpy()[[0, 2, 3]], rlp[[0, 2, 3]], rtol=1e-15, atol=0)
    pi0, lp0 = ml2d.update_priors(np.zeros(3))
    assert not pi0.any() and (lp0 == -math.inf).all()
    ll = ml2d.log_likelihood(torch.from_numpy(lse), torch.from_numpy(live), C, n, 0.37, A, S)
    want = lse[live].sum() - live.sum() * (C * n * n / 2) * math.log(2 * math.pi * 0.37) - live.sum() * math.log(7 * 25)
    assert ll == pytest.approx(want, rel=1e-14) and ll == pytest.approx(ml_ref.log_likelihood(lse, live, C, n, 0.37, A, S), rel=1e-14)
    resp = np.array([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.25, 0.25, 0.5]], dtype=F32)
    ent = ml2d.class_entropy(torch.from_numpy(resp)).numpy()
    assert np.allclose(ent, [math.log(2), 0.0, 0.0, 1.5 * math.log(2)], rtol=1e-15, atol=0)
    # the smallest live residual
    num, pp, yy, cand = random_tables(rng, 5, 2, 1, 1, 3)
    cand[0] = -1
    num[1, 0, 0, 0, 0] = np.nan
    got = ml2d.min_residuals(torch.from_numpy(num), torch.from_numpy(pp), torch.from_numpy(yy), torch.from_numpy(cand), 3).numpy()
    l, r = ml_ref.log_weights(num, pp, yy, cand, None, 3, 1.0)
    assert np.array_equal(got, np.where(np.isnan(l), np.inf, r).min(1)) and got[0] == np.inf


# ---- the parser ------------------------------------------------------------------------------------------------------------------
def _flags(p):
    return sorted(s for a in p._actions for s in a.option_strings if a.dest != 'help')


def test_parser_and_script():
    from tvae import classify, ml2d
    p = ml2d.build_parser()
    assert _flags(p) == sorted(_flags(classify.build_parser()) + ['--keep', '--sigma2'])
    need = ['--stack', 's.npy', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy']
    a = p.parse_args(need)
    assert (a.keep, a.sigma2, a.rounds, a.angle_range, a.angle_steps, a.shift, a.cross_halves) == (8, None, 3, 22.5, 8, 2, False)
    assert a.latents is None and a.candidates is None and (a.t_inf, a.out_dir, a.device) == ('attention', '.', 0)
    a = p.parse_args(need + ['--keep', '4', '--sigma2', '0.5', '--cross-halves', '--candidates', '3', '--latents', 'z.npy'])
    assert (a.keep, a.sigma2, a.cross_halves, a.candidates, a.latents) == (4, 0.5, True, 3, 'z.npy')
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's.npy'])
    assert '--keep' not in _flags(classify.build_parser())    # the parser it borrows from is what it was
    spec = importlib.util.spec_from_file_location('ml_class_averages_script', os.path.join(PKG, 'ml_class_averages.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run is ml2d.run and callable(mod.main)
    spec = importlib.util.spec_from_file_location('ml_bench', os.path.join(ROOT, 'profiles', 'tools', 'ml_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    b = mod.build_parser().parse_args([])
    assert b.shapes == ['100000x64', '20000x128'] and (b.clusters, b.candidates, b.angle_steps, b.shift, b.keep, b.reps) == (10, 4, 8, 2, 8, 10)


# ---- the loop, by the reference alone --------------------------------------------------------------------------------------------
def test_reference_loop_has_a_clear_cut_at_the_kept_entries():
    """The GPU test compares sigma^2 and the log-likelihood of every round with this reference: its own top-P sets must not
    hang on a near tie.  No kept candidate is within 1e-6 in weight of one that is not."""
    p, r = ml_ref.loop_reference()
    print('ml_ref.rounds: gaps', r['gaps'], 'sigma2', r['sigma2'], 'log-likelihood', r['log_likelihood'], 'kept', r['kept'])
    assert (r['gaps'] >= 1e-6).all()
    assert np.isfinite(r['log_likelihood']).all() and (r['sigma2'] > 0).all() and r['pi'].shape == (2, p['K'])
    assert np.allclose(r['pi'].sum(1), 1.0, rtol=0, atol=1e-12) and abs(r['wsum'].sum() - 24) <= 24 * 2.0 ** -22
