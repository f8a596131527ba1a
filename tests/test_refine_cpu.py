"""Pose refinement against the class averages, the part that needs no GPU: the fp64 restatement tests/pose_ref.py itself (the
template at the axis angles, the inverse-map round trip that pins the sign of the dx update, the selection rule), the
cross-half assignment against the even / odd rule of tests/frc_ref.py, the halving of the angle step in refine_rounds, the
parsers, and the header against the binding for the new names."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import align_ref
import frc_ref
import pose_ref
from conftest import PKG, ROOT


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_template_at_the_axis_angles_is_a_permutation_of_the_reference():
    """theta a multiple of pi / 2 and whole-pixel dx: the pixel (r, q) reads the reference at a whole pixel.  theta = 0 is exact;
    the fp32 values of pi / 2 and pi are off by up to 9e-8, so those agree within that times the side times the largest
    adjacent step."""
    n = 9
    rng = np.random.default_rng(3)
    ref = rng.standard_normal((1, 1, n, n)).astype(np.float32)
    h = 2.0 / (n - 1)
    c = (n - 1) // 2
    step = max(np.abs(np.diff(ref, axis=2)).max(), np.abs(np.diff(ref, axis=3)).max())
    for quarter in range(4):
        for sx, sy in ((0, 0), (2, -1)):                      # the content moves sx pixels right and sy pixels down
            theta = np.array([quarter * np.pi / 2], dtype=np.float32)
            dx = np.array([[sx * h, -sy * h]], dtype=np.float32)
            T = pose_ref.templates(ref, [0], theta, dx, 1.0, 0, 0.0, 0)[0, 0, 0]
            want = np.zeros((n, n))
            hit = np.zeros((n, n), dtype=int)
            cs, sn = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarter]
            for r in range(n):
                for q in range(n):
                    v0, v1 = (q - sx) - c, c - (r - sy)       # in pixels from the centre, x1 upwards
                    u0, u1 = v0 * cs - v1 * sn, v0 * sn + v1 * cs
                    col, row = u0 + c, c - u1
                    if 0 <= col < n and 0 <= row < n:
                        want[r, q] = ref[0, 0, row, col]
                        hit[row, col] += 1
            assert hit.max() == 1 and (hit.sum() == n * n) == ((sx, sy) == (0, 0))        # a permutation; a shift loses a border
            tol = 0.0 if quarter == 0 else 2 * step * 1e-7 * n
            assert np.abs(T - want).max() <= tol, (quarter, sx, sy, np.abs(T - want).max())
    # the extended grid continues the frame: its inner n x n block is the S = 0 template
    T0 = pose_ref.templates(ref, [0], [0.3], [[0.1, -0.2]], 1.0, 1, 0.1, 0)
    T2 = pose_ref.templates(ref, [0], [0.3], [[0.1, -0.2]], 1.0, 1, 0.1, 2)
    assert T2.shape == (1, 3, 1, n + 4, n + 4) and np.array_equal(T2[..., 2:-2, 2:-2], T0)


def test_tables_scores_and_hostile_inputs():
    n, S, A = 8, 1, 1
    rng = np.random.default_rng(5)
    refs = rng.standard_normal((2, 2, n, n)).astype(np.float32)
    Y = rng.standard_normal((5, 2, n, n)).astype(np.float32)
    theta = np.array([0.2, np.nan, 0.1, -0.4, 1.0], dtype=np.float32)
    dx = np.array([[0.1, 0.0], [0.0, 0.0], [np.inf, 0.0], [0.0, 0.1], [0.0, 0.0]], dtype=np.float32)
    cls = np.array([0, 1, 1, 2, -1])
    Y[0] = 0.0                                               # yy = 0: every score is an exact 0
    res = pose_ref.refine(Y, theta, dx, cls, refs, 1.0, A, 0.1, S)
    assert res['num'].shape == (5, 3, 3, 3) and res['score'].dtype == np.float32
    assert not res['T'][1:].any() and not res['num'][1:].any() and not res['pp'][1:].any()      # hostile poses and skipped images
    assert not res['score'].any() and not res['best'].any() and not res['out'].any()
    assert np.array_equal(res['theta'].view(np.int32), theta.view(np.int32)) and np.array_equal(res['dx'].view(np.int32), dx.view(np.int32))
    # the direct form of one candidate: every pixel of the frame reads the template of the shifted pose
    Y[0] = rng.standard_normal((2, n, n))
    res = pose_ref.refine(Y, theta, dx, cls, refs, 1.0, A, 0.1, S)
    a, sy, sx = 1, -1, 1
    th = np.float32(theta[0] + np.float32(a) * np.float32(0.1))
    moved = dx[0].astype(np.float64) + np.array([2 * sx / (n - 1), -2 * sy / (n - 1)])
    P = pose_ref.templates(refs, [0], [th], [moved], 1.0, 0, 0.0, 0)[0, 0]
    assert np.abs(res['num'][0, a + A, sy + S, sx + S] - (P * Y[0]).sum()) <= 1e-12 * np.abs(P * Y[0]).sum()
    assert np.abs(res['pp'][0, a + A, sy + S, sx + S] - (P * P).sum()) <= 1e-12 * (P * P).sum()
    assert res['out'][0, 1] >= res['out'][0, 0] and np.abs(res['score'][0]).max() <= 1 + 1e-6


def test_selection_rule():
    sc = np.zeros((4, 3, 3, 3), dtype=np.float32)
    sc[0, 1, 1, 1], sc[0, 0, 2, 2], sc[0, 2, 0, 0] = 0.5, 0.7, 0.7        # a tie: the first in ascending (a, sy, sx) stays
    sc[1] = np.nan                                                        # nothing finite: unchanged, scores 0
    sc[2, 1, 1, 1], sc[2, 2, 2, 2] = np.nan, -0.3                         # a centre that is not finite counts as -inf
    sc[3, 1, 1, 1], sc[3, 0, 0, 0] = 0.4, np.inf                          # inf is not finite: never chosen
    best, out = pose_ref.select(sc, [0, 0, 0, 5], 1)
    assert best.tolist() == [[-1, 1, 1], [0, 0, 0], [-1, -1, -1], [0, 0, 0]]
    assert out[0].tolist() == [0.5, np.float32(0.7)] and out[1].tolist() == [0, 0] and out[3].tolist() == [0, 0]
    assert out[2, 0] == -np.inf and out[2, 1] == 0.0
    th, dx = pose_ref.update_pose(np.float32([-0.0, 1, 2, 3]), np.float32([[-0.0, 5], [1, 1], [2, 2], [3, 3]]), best, 9, 0.5, 0.25)
    assert th.tolist() == [-0.25, 1, 1.75, 3]
    assert dx.tolist() == [[0.5, 4.5], [1, 1], [1.5, 2.5], [3, 3]]        # dx' = dx + (2 sx, -2 sy) / (n - 1) / t


def test_inverse_map_round_trip_recovers_every_planted_pose():
    """Pins the sign of the dx update: the images show the references at (theta_true, dx_true), the start is off by a planted
    candidate, and the fp64 selection must return that candidate -- and with it the true pose -- for EVERY image."""
    p = pose_ref.planted()
    res = pose_ref.refine(p['Y'], p['theta'], p['dx'], p['cls'], p['refs'], p['t'], p['A'], p['dtheta'], p['S'])
    assert np.array_equal(res['best'], p['want']), np.flatnonzero((res['best'] != p['want']).any(1))
    assert (res['out'][:, 1] > 1 - 1e-5).all() and (res['out'][:, 1] >= res['out'][:, 0]).all()
    assert np.abs(res['theta'].astype(np.float64) - p['theta_true']).max() <= 4e-7 * np.pi
    assert np.abs(res['dx'].astype(np.float64) - p['dx_true']).max() <= 4e-7
    keep = np.flatnonzero((p['want'] == 0).all(1))
    assert keep.size and np.array_equal(res['theta'][keep].view(np.int32), p['theta'][keep].view(np.int32))
    assert np.array_equal(res['dx'][keep].view(np.int32), p['dx'][keep].view(np.int32))
    # the other sign of either shift does not come back
    wrong = pose_ref.update_pose(p['theta'], p['dx'], p['want'] * [1, -1, 1], p['n'], p['t'], p['dtheta'])[1]
    moved = p['want'][:, 1] != 0
    assert (np.abs(wrong[moved, 1].astype(np.float64) - p['dx_true'][moved, 1]) > 1.0 / p['n']).all()
    # t = 0.1: the same candidates with the translations in the unimodal encoder's units
    q = pose_ref.planted(t=0.1)
    res = pose_ref.refine(q['Y'], q['theta'], q['dx'], q['cls'], q['refs'], q['t'], q['A'], q['dtheta'], q['S'])
    assert np.array_equal(res['best'], q['want'])


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def test_cross_half_assignment_is_the_even_odd_rule():
    from tvae import refine
    rng = np.random.default_rng(11)
    K = 4
    labels = rng.integers(-1, K + 1, 57)
    labels[labels == 2] = 0                                   # an empty class
    got = refine.cross_half_labels(torch.from_numpy(labels), K).numpy()
    assert np.array_equal(got, pose_ref.cross_half_labels(labels, K))
    order, seg, _ = align_ref.segments(labels, K)
    for k, (even, odd) in enumerate(frc_ref.half_lists(order, seg, labels.size)):
        assert (got[even] == K + k).all() and (got[odd] == k).all()      # half 0 is scored against half 1 and the reverse
    assert (got[(labels < 0) | (labels >= K)] == -1).all() and not (got == 2).any() and not (got == K + 2).any()


def test_refine_rounds_halves_the_angle_step(monkeypatch):
    from tvae import _cluster_lib as CL, align, refine
    monkeypatch.setattr(CL, 'is_f32', lambda t, contiguous=True: True)
    seen = []

    def fake_refine(images, theta, dx, labels, refs, t_scale, A, step, shift, mask_radius, mask_edge):
        seen.append((A, step, shift, refs.shape[0], labels.tolist()))
        return theta + 1, dx, torch.full((images.shape[0], 2), float(len(seen))), None

    monkeypatch.setattr(refine, 'refine_poses', fake_refine)
    monkeypatch.setattr(align, 'class_averages', lambda im, th, dx, lab, K, t: (torch.zeros(K, 1, 4, 4), None))
    monkeypatch.setattr(align, 'class_halves', lambda im, th, dx, lab, K, t: (None, torch.zeros(2, K, 1, 4, 4), None, None))
    Y, th, dx = torch.zeros(6, 1, 4, 4), torch.zeros(6), torch.zeros(6, 2)
    lab = np.array([0, 1, 0, 0, 2, 1])
    out = refine.refine_rounds(Y, th, dx, lab, 2, rounds=3, angle_range=0.4, angle_steps=4, shift=1)
    assert [s[1] for s in seen] == [0.1, 0.05, 0.025] == out[2]['steps'] and [s[0] for s in seen] == [4, 4, 4]
    assert [s[3] for s in seen] == [2, 2, 2] and seen[0][4] == lab.tolist()
    assert out[0].tolist() == [3.0] * 6 and out[2]['scores'].tolist() == [[1, 1], [2, 2], [3, 3]]
    seen.clear()
    refine.refine_rounds(Y, th, dx, lab, 2, rounds=1, cross_halves=True)
    assert seen[0][3] == 4 and seen[0][4] == [2, 3, 0, 2, -1, 1] and seen[0][1] == pytest.approx(np.pi / 8 / 8)
    from tvae._lib import TvaeHipError
    with pytest.raises(TvaeHipError, match='rounds'):
        refine.refine_rounds(Y, th, dx, lab, 2, rounds=0)


def test_refine_poses_argument_checks(monkeypatch):
    from tvae import _cluster_lib as CL, refine
    from tvae._lib import TvaeHipError
    Y, th, dx = torch.zeros(3, 1, 8, 8), torch.zeros(3), torch.zeros(3, 2)
    lab, refs = torch.zeros(3, dtype=torch.int64), torch.zeros(2, 1, 8, 8)
    with pytest.raises(TvaeHipError, match='no CPU fallback'):            # the messages of tvae.align
        refine.refine_poses(Y, th, dx, lab, refs)
    monkeypatch.setattr(CL, 'is_f32', lambda t, contiguous=True: True)
    big = torch.zeros(1, 1, 130, 130)
    with pytest.raises(TvaeHipError, match='tvae.image'):
        refine.refine_poses(big, th[:1], dx[:1], lab[:1], big)
    for kw in (dict(angle_steps=33), dict(shift=9), dict(shift=-1), dict(t_scale=0.0), dict(angle_step=float('nan')),
               dict(mask_edge=-1.0), dict(mask_radius=float('inf'))):
        with pytest.raises(TvaeHipError):
            refine.refine_poses(Y, th, dx, lab, refs, **kw)
    with pytest.raises(TvaeHipError, match='labels must hold'):
        refine.refine_poses(Y, th, dx, lab[:2], refs)
    with pytest.raises(TvaeHipError, match='refs must be'):
        refine.refine_poses(Y, th, dx, lab, refs[:, :, :4])


def _flags(p):
    return sorted(s for a in p._actions for s in a.option_strings if a.dest != 'help')


def test_parsers():
    from tvae import align, refine
    p = refine.build_parser()
    assert _flags(p) == sorted(['--stack', '--rotations', '--translations', '--clusters', '--t-inf', '--crop', '--n-clusters',
                                '--out-dir', '-d', '--device', '--rounds', '--angle-range', '--angle-steps', '--shift',
                                '--mask-radius', '--mask-edge', '--cross-halves'])
    need = ['--stack', 's.npy', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy']
    a = p.parse_args(need)
    assert (a.t_inf, a.crop, a.n_clusters, a.out_dir, a.device) == ('attention', 0, None, '.', 0)
    assert (a.rounds, a.angle_range, a.angle_steps, a.shift, a.mask_radius, a.mask_edge, a.cross_halves) == (3, 22.5, 8, 2, None, 0.0, False)
    a = p.parse_args(need + ['--rounds', '2', '--angle-range', '10', '--angle-steps', '4', '--shift', '3', '--mask-radius', '12',
                             '--mask-edge', '3', '--cross-halves', '--t-inf', 'unimodal', '-d', '1'])
    assert (a.rounds, a.angle_range, a.angle_steps, a.shift, a.mask_radius, a.mask_edge, a.cross_halves) == (2, 10.0, 4, 3, 12.0, 3.0, True)
    assert (a.t_inf, a.device) == ('unimodal', 1)
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's.npy'])
    # the parser it borrows from is what it was
    assert '--write-aligned' in _flags(align.build_parser()) and '--rounds' not in _flags(align.build_parser())
    spec = importlib.util.spec_from_file_location('refine_poses_script', os.path.join(PKG, 'refine_poses.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run is refine.run and callable(mod.main)
    spec = importlib.util.spec_from_file_location('refine_bench', os.path.join(ROOT, 'profiles', 'tools', 'refine_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    b = mod.build_parser()
    assert _flags(b) == sorted(['--shapes', '--clusters', '--angle-steps', '--shifts', '--reps', '--warmup', '--out',
                                '--skip-route', '--tag'])
    a = b.parse_args([])
    assert a.shapes == ['100000x64', '20000x128'] and a.clusters == 10 and a.angle_steps == 8 and a.shifts == [2, 3]
    assert a.reps == 10 and mod.parse_shape('20000x128') == (20000, 128)
    assert mod.multiply_adds(64, 1, 8, 3) == 17 * 49 * 64 * 64


# ---- header, binding, queries ----------------------------------------------------------------------------------------------
NEW_CALLS = {'tvae_pose_refine': 'ppppp' 'pppp' 'ppp' 'p' 'l' 'iiiiii' 'ffff'}
NEW_QUERIES = {'tvae_pose_refine_ws_floats': ('iiiii', 'l')}


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
    assert {n for n in declared if 'refine' in n} == set(NEW_CALLS) | set(NEW_QUERIES)      # exactly the new symbols
    L = CL.lib()
    assert L.tvae_cluster_abi_version() == 1
    for name in list(NEW_CALLS) + list(NEW_QUERIES):
        assert hasattr(L, name), name
    flat = ' '.join(hdr.split())
    assert 'visited in ascending (a, sy, sx)' in flat and 'r mod G' in flat and '-2 sy / (n - 1)' in flat


def test_queries():
    from tvae import _cluster_lib as CL
    for N, C, n, A, S in [(1, 1, 2, 0, 0), (24, 3, 32, 8, 2), (3, 1, 128, 2, 3), (1 << 24, 16, 128, 32, 8), (100000, 1, 64, 8, 3)]:
        assert CL.query('tvae_pose_refine_ws_floats', N, C, n, A, S) == N * (2 * (2 * A + 1) * (2 * S + 1) ** 2 + 1)
    for bad in [(0, 1, 8, 1, 1), (-3, 1, 8, 1, 1), ((1 << 24) + 1, 1, 8, 1, 1), (4, 0, 8, 1, 1), (4, 17, 8, 1, 1), (4, 1, 1, 1, 1),
                (4, 1, 129, 1, 1), (4, 1, 8, -1, 1), (4, 1, 8, 33, 1), (4, 1, 8, 1, -1), (4, 1, 8, 1, 9)]:
        assert CL.query('tvae_pose_refine_ws_floats', *bad) == 0, bad
