"""Reassignment against the class averages, the part that needs no GPU: the header against the binding for the new names and
the workspace query, the parsers of reclassify_particles.py and classify_bench.py, tvae.classify.candidate_lists and the
cross-half slot rule against tests/classify_ref.py, the rule across slots on hand-made score tables, and recovery by the fp64
reference alone -- the condition the GPU tests lean on."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import classify_ref
import pose_ref
from conftest import PKG, ROOT


# ---- header, binding, queries ----------------------------------------------------------------------------------------------
NEW_CALLS = {'tvae_pose_classify': 'ppppp' 'ppppp' 'ppp' 'p' 'l' 'iiiiiii' 'ffff'}
NEW_QUERIES = {'tvae_pose_classify_ws_floats': ('iiiiii', 'l')}


def test_header_and_binding_of_the_new_entry_points():
    from tvae import _cluster_lib as CL
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
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
        assert m and m.group(1) == {'i': 'int', 'l': 'long'}[ret]
        assert all(a.strip().startswith('int ') for a in m.group(2).split(',')) and len(m.group(2).split(',')) == len(sig)
    declared = set(re.findall(r'\b(?:int|long)\s+(tvae_\w+)\s*\(', hdr))
    assert {n for n in declared if 'classify' in n} == set(NEW_CALLS) | set(NEW_QUERIES)      # exactly the new symbols
    assert re.search(r'#define\s+TVAE_CLASSIFY_MAX_CANDIDATES\s+64\b', hdr)
    L = CL.lib()
    assert L.tvae_cluster_abi_version() == 1
    for name in list(NEW_CALLS) + list(NEW_QUERIES):
        assert hasattr(L, name), name
    flat = ' '.join(hdr.split())
    assert 'visited in ascending m' in flat and 'strictly greater' in flat and 'cls_out[i] = cand[i][m*]' in flat


def test_queries():
    from tvae import _cluster_lib as CL
    for N, M, C, n, A, S in [(1, 1, 1, 2, 0, 0), (24, 4, 3, 32, 8, 2), (3, 2, 1, 128, 2, 3), (1 << 24, 64, 16, 128, 32, 8),
                             (100000, 10, 1, 64, 8, 2)]:
        assert CL.query('tvae_pose_classify_ws_floats', N, M, C, n, A, S) == N * (2 * M * (2 * A + 1) * (2 * S + 1) ** 2 + 1)
    for bad in [(4, 0, 1, 8, 1, 1), (4, 65, 1, 8, 1, 1), (4, -1, 1, 8, 1, 1), (0, 2, 1, 8, 1, 1), ((1 << 24) + 1, 2, 1, 8, 1, 1),
                (4, 2, 0, 8, 1, 1), (4, 2, 17, 8, 1, 1), (4, 2, 1, 1, 1, 1), (4, 2, 1, 129, 1, 1), (4, 2, 1, 8, -1, 1),
                (4, 2, 1, 8, 33, 1), (4, 2, 1, 8, 1, -1), (4, 2, 1, 8, 1, 9)]:
        assert CL.query('tvae_pose_classify_ws_floats', *bad) == 0, bad


# ---- parsers -----------------------------------------------------------------------------------------------------------------
def _flags(p):
    return sorted(s for a in p._actions for s in a.option_strings if a.dest != 'help')


def test_parsers():
    from tvae import classify, refine
    p = classify.build_parser()
    assert _flags(p) == sorted(_flags(refine.build_parser()) + ['--latents', '--candidates'])
    need = ['--stack', 's.npy', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy']
    a = p.parse_args(need)
    assert (a.t_inf, a.crop, a.n_clusters, a.out_dir, a.device) == ('attention', 0, None, '.', 0)
    assert (a.rounds, a.angle_range, a.angle_steps, a.shift, a.mask_radius, a.mask_edge, a.cross_halves) == (3, 22.5, 8, 2, None, 0.0, False)
    assert a.latents is None and a.candidates is None
    a = p.parse_args(need + ['--latents', 'z.npy', '--candidates', '4', '--rounds', '2', '--cross-halves'])
    assert (a.latents, a.candidates, a.rounds, a.cross_halves) == ('z.npy', 4, 2, True)
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's.npy'])
    assert '--latents' not in _flags(refine.build_parser())              # the parser it borrows from is what it was
    spec = importlib.util.spec_from_file_location('reclassify_particles_script', os.path.join(PKG, 'reclassify_particles.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run is classify.run and callable(mod.main)
    spec = importlib.util.spec_from_file_location('classify_bench', os.path.join(ROOT, 'profiles', 'tools', 'classify_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    b = mod.build_parser()
    assert _flags(b) == sorted(['--shapes', '--clusters', '--candidates', '--angle-steps', '--shift', '--reps', '--warmup',
                                '--parent-lib', '--tag', '--out'])
    a = b.parse_args([])
    assert a.shapes == ['100000x64', '20000x128'] and a.clusters == 10 and a.candidates == [10, 4]
    assert (a.angle_steps, a.shift, a.reps, a.warmup, a.parent_lib) == (8, 2, 10, 2, None)
    assert mod.parse_shape('20000x128') == (20000, 128)


# ---- candidate lists -----------------------------------------------------------------------------------------------------------
def test_candidate_lists_without_latents():
    from tvae import classify
    rng = np.random.default_rng(4)
    K = 5
    labels = rng.integers(-1, K + 1, 40)
    labels[labels == 3] = 1                                   # an empty class
    got = classify.candidate_lists(torch.from_numpy(labels), K)
    assert got.dtype == torch.int64 and tuple(got.shape) == (40, K)
    got = got.numpy()
    assert np.array_equal(got, classify_ref.candidate_lists(labels, K))
    member = (labels >= 0) & (labels < K)
    assert member.any() and (~member).any()
    assert np.array_equal(got[member, 0], labels[member]) and (got[~member, 0] == -1).all()
    for i in np.flatnonzero(member):                          # every class exactly once, the others ascending
        assert sorted(got[i]) == list(range(K)) and list(got[i, 1:]) == sorted(got[i, 1:])
    assert np.array_equal(classify.candidate_lists(labels, K, m=3).numpy(), classify_ref.candidate_lists(labels, K, m=3))
    assert classify.candidate_lists(labels, K, m=1).numpy()[:, 0].tolist() == np.where(member, labels, -1).tolist()


def test_candidate_lists_with_latents():
    from tvae import classify
    # centroids on a line at 0, 10, 20, (class 3 empty), 40: whole numbers, so distances and ties are exact
    labels = np.array([0, 0, 1, 1, 2, 2, 4, 4, -1, 9])
    z = np.array([[-1.0, 0], [1, 0], [9, 0], [11, 0], [19, 0], [21, 0], [39, 0], [41, 0], [15, 0], [5, 0]])
    K = 5
    want = classify_ref.candidate_lists(labels, K, z, 4)
    got = classify.candidate_lists(torch.from_numpy(labels), K, torch.from_numpy(z), 4).numpy()
    assert np.array_equal(got, want)
    assert got[0].tolist() == [0, 1, 2, 4] and got[2].tolist() == [1, 0, 2, 4] and got[6].tolist() == [4, 2, 1, 0]
    assert got[8].tolist() == [-1, 1, 2, 0]                   # 15 is as far from 10 as from 20: the tie goes to the lower class
    assert got[9].tolist() == [-1, 0, 1, 2]                   # and 5 as far from 0 as from 10
    full = classify.candidate_lists(labels, K, z.astype(np.float32)).numpy()
    assert np.array_equal(full, classify_ref.candidate_lists(labels, K, z)) and (full[:8, -1] == 3).all()      # the empty class last
    rng = np.random.default_rng(9)
    lab = rng.integers(0, 6, 80)
    zz = rng.standard_normal((80, 3))
    assert np.array_equal(classify.candidate_lists(lab, 6, zz, 3).numpy(), classify_ref.candidate_lists(lab, 6, zz, 3))


def test_candidate_lists_reject():
    from tvae import classify
    from tvae._lib import TvaeHipError
    lab = np.arange(70) % 65
    with pytest.raises(TvaeHipError, match='give m'):
        classify.candidate_lists(lab, 65)
    assert tuple(classify.candidate_lists(lab, 65, m=8).shape) == (70, 8)
    for kw in (dict(m=0), dict(m=6), dict(m=65)):
        with pytest.raises(TvaeHipError):
            classify.candidate_lists(lab % 5, 5 if kw['m'] < 65 else 70, **kw)
    with pytest.raises(TvaeHipError):
        classify.candidate_lists(lab.astype(np.float32), 5)
    with pytest.raises(TvaeHipError, match='latents must be'):
        classify.candidate_lists(lab % 5, 5, np.zeros((3, 2)))


def test_cross_half_slots():
    from tvae import classify
    rng = np.random.default_rng(12)
    K = 4
    labels = rng.integers(-1, K + 1, 31)
    cand = classify_ref.candidate_lists(labels, K)
    cand[3, 2] = 11
    want = classify_ref.cross_half_candidates(labels, cand, K)
    got = classify.cross_half_candidates(torch.from_numpy(labels), torch.from_numpy(cand), K).numpy()
    assert np.array_equal(got, want)
    own = pose_ref.cross_half_labels(labels, K)
    member = own >= 0
    assert np.array_equal(got[member, 0], own[member])        # slot 0: the half that does not contain the image
    assert (got[~member, 0] == -1).all() and got[3, 2] == -1
    valid = (cand >= 0) & (cand < K)
    assert np.array_equal(got[valid] % K, cand[valid])        # % K maps back
    for i in range(31):                                       # one half for the whole row
        assert len({int(v) // K for v in got[i] if v >= 0}) <= 1


# ---- the rule across slots -----------------------------------------------------------------------------------------------------
def test_rule_across_slots():
    K = 4
    cand = np.array([[2, 0, 1], [1, 1, 3], [-1, 2, 0], [-1, 9, 4], [0, 1, 2], [3, 0, -1]])
    out = np.zeros((6, 3, 2), dtype=np.float32)
    sb = np.zeros((6, 3, 3), dtype=np.int64)
    sb[:, :, 0] = [[1, 2, 3]] * 6                             # the slot's candidate names the slot
    out[0, :, 1] = [0.7, 0.7, 0.6]                            # a tie stays with slot 0
    out[1, :, 1] = [0.5, 0.5, 0.4]                            # a duplicate never wins
    out[2, :, 1] = [0.0, -0.3, -0.2]                          # slot 0 skipped: the first valid slot starts, a greater one replaces it
    out[3, :, 1] = [0.0, 0.0, 0.0]                            # all slots skipped
    out[4, :, 1] = [0.0, 0.0, 0.0]                            # all scores 0: slot 0
    out[5, :, 1] = [-0.5, 0.2, 0.9]                           # a skipped slot's figures do not count
    cls, best = classify_ref.choose(out, sb, cand, K)
    assert cls.tolist() == [2, 1, 0, -1, 0, 0]
    assert best[:, 0].tolist() == [0, 0, 2, 0, 0, 1]
    assert best[:, 1].tolist() == [1, 1, 3, 0, 1, 2] and not best[3].any()
    # -inf centre and a slot that reports 0 because nothing was finite competes with that 0
    out2 = np.zeros((1, 2, 2), dtype=np.float32)
    out2[0, 0] = (-np.inf, -0.1)
    cls, best = classify_ref.choose(out2, np.zeros((1, 2, 3), dtype=np.int64), np.array([[0, 1]]), 2)
    assert cls.tolist() == [1] and best[0, 0] == 1


# ---- recovery by the reference alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(seed=7), dict(seed=41, N=24, K=4, n=17, A=2, S=3)])
def test_reference_recovers_the_planted_class_with_a_margin(kw):
    p = pose_ref.planted(**kw)
    K = p['K']
    cand = classify_ref.candidate_lists(p['cls'], K)
    res = classify_ref.classify(p['Y'], p['theta'], p['dx'], cand, p['refs'], p['t'], p['A'], p['dtheta'], p['S'])
    sb = res['score'][:, :, 1].astype(np.float64)
    margin = sb[:, 0] - sb[:, 1:].max(1)                      # slot 0 is the true class
    print('classify_ref: least margin of the true class', margin.min())
    assert margin.min() >= 0.05
    assert np.array_equal(res['cls'], p['cls']) and np.array_equal(res['best'][:, 1:], p['want']) and not res['best'][:, 0].any()
    # with a wrong class in slot 0 for every third image the true class still wins, from its own slot
    start = mislabel(p)
    cand = classify_ref.candidate_lists(start, K)
    res = classify_ref.classify(p['Y'], p['theta'], p['dx'], cand, p['refs'], p['t'], p['A'], p['dtheta'], p['S'])
    assert np.array_equal(res['cls'], p['cls']) and np.array_equal(res['best'][:, 1:], p['want'])
    assert (res['best'][::3, 0] > 0).all()


def mislabel(p):
    """The planted labels with a wrong class for every third image."""
    start = p['cls'].copy()
    start[::3] = (start[::3] + 1) % p['K']
    return start


def rounds_start():
    """The blurred start of test_refine_gpu.py with every third image in a wrong class: planted(seed=21, N=60), default_rng(22)
    drawing the +-10 degree and +-2 px errors in that order and then the wrong labels."""
    p = pose_ref.planted(seed=21, N=60)
    rng = np.random.default_rng(22)
    n, K = p['n'], p['K']
    theta0 = (p['theta_true'] + np.radians(rng.uniform(-10, 10, 60))).astype(np.float32)
    dx0 = (p['dx_true'] + rng.uniform(-2, 2, (60, 2)) * 2 / (n - 1)).astype(np.float32)
    labels0 = p['cls'].copy()
    third = np.arange(60) % 3 == 0
    labels0[third] = (p['cls'][third] + 1 + rng.integers(0, K - 1, int(third.sum()))) % K
    return p, theta0, dx0, labels0


def test_reference_rounds_end_with_no_wrong_label():
    p, theta0, dx0, labels0 = rounds_start()
    K = p['K']
    assert (labels0 != p['cls']).sum() == 20
    lab, th, d, hist = classify_ref.rounds(p['Y'], theta0, dx0, labels0, K, 1.0, rounds=3, angle_range=np.pi / 8, A=8, S=2)
    wrong = [int((labels0 != p['cls']).sum())]
    print('classify_ref.rounds: moved', hist['moved'].tolist(), 'scores', hist['scores'].tolist())
    assert np.array_equal(lab, p['cls']) and hist['moved'][-1] == 0
    assert np.array_equal(hist['counts'][-1], np.bincount(p['cls'], minlength=K)) and hist['counts'].shape == (4, K)
    assert (np.diff(hist['scores'][:, 1]) >= 0).all() and hist['steps'] == [np.pi / 64, np.pi / 128, np.pi / 256]
    sb = hist['slot_scores'][:, :, 1].astype(np.float64)
    top = np.sort(sb, 1)
    assert (top[:, -1] - top[:, -2]).min() >= 0.05 and wrong[0] == 20
