"""The host scaffold of the class-average tools (tvae.stack_cli) and the one statement of the pose-search argument rules
(tvae.refine), the part that needs no GPU: the seven parsers against the record of what they declared before the scaffold
existed (tests/golden/cli_flags_class_tools.json), the inputs opened on the CPU, the argument checks of the three pose
searches through their public functions, the references of a round, the resolution table, the files every pose family
writes and the hand-off of the refined poses to the polish in the driver.

    python tests/test_stack_cli_cpu.py --record     writes the golden again from the parsers as they are
"""
import contextlib
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG

PARSERS_JSON = os.path.join(GOLDEN, 'cli_flags_class_tools.json')
NEED = ['--stack', 's.npy', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy']


def _parsers():
    from tvae import align, classify, eigen, ml2d, polish, refine, resolution
    out = {}
    for name, mod in (('align', align), ('resolution', resolution), ('eigen', eigen)):
        out[name] = mod.build_parser()
        out[name + '+ctf'] = mod.build_parser(ctf=True)
    for name, mod in (('refine', refine), ('polish', polish), ('classify', classify), ('ml2d', ml2d)):
        out[name] = mod.build_parser()
    return out


def _snapshot(parser):
    """prog and, for every action except help in order, what argparse was told about it."""
    return dict(prog=parser.prog, actions=[
        dict(flags=list(a.option_strings), dest=a.dest, default=a.default, type=getattr(a.type, '__name__', None),
             choices=list(a.choices) if a.choices else None, required=a.required, nargs=a.nargs, help=a.help)
        for a in parser._actions if a.dest != 'help'])


# ---- 1. the parsers ----------------------------------------------------------------------------------------------------------
def test_every_parser_is_what_it_was():
    want = json.load(open(PARSERS_JSON))
    got = {k: _snapshot(p) for k, p in _parsers().items()}
    assert sorted(got) == sorted(want) and len(want) == 10
    for name in want:
        assert got[name]['prog'] == want[name]['prog'], name
        assert [a['dest'] for a in got[name]['actions']] == [a['dest'] for a in want[name]['actions']], name
        for a, b in zip(got[name]['actions'], want[name]['actions']):
            assert a == b, (name, a['dest'])


def test_no_module_reaches_into_argparse():
    pkg = os.path.join(PKG, 'tvae')
    for f in sorted(os.listdir(pkg)):
        if f.endswith('.py'):
            src = open(os.path.join(pkg, f)).read()
            assert '_add_action' not in src and '._actions' not in src, f


# ---- 2. opening the inputs ------------------------------------------------------------------------------------------------------
def _write_inputs(d, stack_name='stack.npy'):
    rng = np.random.default_rng(2)
    stack = rng.standard_normal((5, 6, 6))
    if stack_name.endswith('.npy'):
        np.save(d / stack_name, stack)
    else:
        from src import mrc
        with open(d / stack_name, 'wb') as f:
            mrc.write(f, stack.astype(np.float32))
    np.save(d / 'rot.npy', rng.standard_normal((5, 1)))
    np.save(d / 'tr.npy', rng.standard_normal((5, 2)))
    np.save(d / 'cl.npy', np.array([[0], [1], [0], [-1], [1]]))
    np.save(d / 'z.npy', rng.standard_normal((5, 3)).astype(np.float32))
    argv = ['--stack', str(d / stack_name), '--rotations', str(d / 'rot.npy'), '--translations', str(d / 'tr.npy'), '--clusters',
            str(d / 'cl.npy')]
    return stack, argv


def test_open_inputs_on_the_cpu(tmp_path):
    from tvae import classify, refine, stack_cli
    cpu = torch.device('cpu')
    stack, argv = _write_inputs(tmp_path)
    inp = stack_cli.open_inputs(refine.build_parser().parse_args(argv + ['--t-inf', 'unimodal']), cpu)
    assert tuple(inp.images.shape) == (5, 1, 6, 6) and inp.images.dtype == torch.float32 and inp.images.is_contiguous()
    assert np.array_equal(inp.images[:, 0].numpy(), stack.astype(np.float32))
    assert tuple(inp.theta.shape) == (5,) and inp.theta.dtype == torch.float32 and inp.rot_shape == (5, 1)
    assert np.array_equal(inp.theta.numpy(), np.load(tmp_path / 'rot.npy').astype(np.float32).reshape(-1))
    assert tuple(inp.dx.shape) == (5, 2) and inp.dx.dtype == torch.float32 and inp.dx.is_contiguous()
    assert inp.clusters.tolist() == [0, 1, 0, -1, 1] and inp.latents is None and inp.particles is False
    assert inp.t_scale == 0.1
    inp = stack_cli.open_inputs(classify.build_parser().parse_args(argv + ['--crop', '4', '--latents', str(tmp_path / 'z.npy')]), cpu)
    assert tuple(inp.images.shape) == (5, 1, 4, 4) and inp.images.is_contiguous() and inp.t_scale == 1.0
    assert np.array_equal(inp.images[:, 0].numpy(), stack.astype(np.float32)[:, 1:5, 1:5])      # one offset per axis
    assert inp.latents.dtype == np.float64 and inp.latents.shape == (5, 3)
    np.save(tmp_path / 'wide.npy', np.zeros((2, 6, 9)))
    argv[1] = str(tmp_path / 'wide.npy')
    inp = stack_cli.open_inputs(refine.build_parser().parse_args(argv + ['--crop', '4']), cpu)
    assert tuple(inp.images.shape) == (2, 1, 4, 4)
    np.save(tmp_path / 'flat.npy', np.zeros((6, 6)))
    argv[1] = str(tmp_path / 'flat.npy')
    with pytest.raises(SystemExit, match=re.escape('--stack must hold [N][n][n] or [N][C][n][n], got (6, 6)')):
        stack_cli.open_inputs(refine.build_parser().parse_args(argv), cpu)


@pytest.mark.parametrize('name,particles', [('stack.mrc', True), ('stack.mrcs', True), ('stack_mrcs.npy', False)])
def test_particles_are_told_by_the_file_name(tmp_path, name, particles):
    from tvae import refine, stack_cli
    stack, argv = _write_inputs(tmp_path, name)
    inp = stack_cli.open_inputs(refine.build_parser().parse_args(argv), torch.device('cpu'))
    assert inp.particles is particles and np.array_equal(inp.images[:, 0].numpy(), stack.astype(np.float32))


def test_no_cpu_compute_path():
    from tvae import refine, stack_cli
    with pytest.raises(SystemExit, match='the MI355X build has no CPU compute path'):
        stack_cli.make_device(refine.build_parser().parse_args(NEED + ['-d', '-1']))
    with pytest.raises(SystemExit, match='^refine_poses: nothing$'):
        with stack_cli.hip_errors():
            from tvae._lib import TvaeHipError
            raise TvaeHipError('refine_poses: nothing')


# ---- 3. the pose-search checks, through the three public functions ----------------------------------------------------------------
BAD = (dict(angle_steps=33), dict(shift=9), dict(shift=-1), dict(t_scale=0.0), dict(angle_step=float('nan')),
       dict(mask_edge=-1.0), dict(mask_radius=float('inf')))          # tests/test_refine_cpu.py::test_refine_poses_argument_checks
GRID = {'refine_poses', 'classify_poses'}                             # the functions that have angle_steps, angle_step and shift


def _searches():
    from tvae import classify, polish, refine
    return (('refine_poses', refine.refine_poses, lambda lab: lab), ('classify_poses', classify.classify_poses, lambda lab: lab[:, None]),
            ('polish_poses', polish.polish_poses, lambda lab: lab))


def test_pose_search_argument_checks(monkeypatch):
    from tvae import _cluster_lib as CL
    from tvae._lib import TvaeHipError
    monkeypatch.setattr(CL, 'is_f32', lambda t, contiguous=True: True)
    seen = []
    monkeypatch.setattr(CL, 'call', lambda name, *a: seen.append((name, a)))
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: contextlib.nullcontext())
    Y, th, dx = torch.zeros(3, 1, 8, 8), torch.zeros(3), torch.zeros(3, 2)
    refs, big = torch.zeros(2, 1, 8, 8), torch.zeros(1, 1, 130, 130)
    lab = torch.tensor([-7, 1, 1 << 40])
    for name, fn, shape in _searches():
        for kw in BAD:
            if name in GRID or set(kw) <= {'t_scale', 'mask_edge', 'mask_radius'}:
                with pytest.raises(TvaeHipError) as e:
                    fn(Y, th, dx, shape(lab), refs, **kw)
                assert str(e.value).startswith(name + ': '), (name, kw, str(e.value))
        with pytest.raises(TvaeHipError, match='tvae.image') as e:
            fn(big, th[:1], dx[:1], shape(lab[:1]), big)
        assert str(e.value).startswith(f'{name}: n = 130 is above 128')
        assert ('must fit the LDS' in str(e.value)) == (name != 'polish_poses')
        with pytest.raises(TvaeHipError, match='refs must be') as e:
            fn(Y, th, dx, shape(lab), refs[:, :, :4])
        assert str(e.value).startswith(name + ': ')
        with pytest.raises(TvaeHipError, match=r'C=17.* outside the supported range \(C <= 16') as e:
            fn(torch.zeros(3, 17, 8, 8), th, dx, shape(lab), torch.zeros(2, 17, 8, 8))
        assert str(e.value).startswith(name + ': ')
        for wrong in (lab.double(), lab > 0):
            with pytest.raises(TvaeHipError, match='integer array') as e:
                fn(Y, th, dx, shape(wrong), refs)
            assert str(e.value).startswith(name + ': ')
        assert not seen                                       # nothing was launched by a rejected call
        fn(Y, th, dx, shape(lab), refs)
        cls = seen[0][1][3]                                # (Y, theta, dx, cls or cand, ...)
        assert seen[0][0] == {'refine_poses': 'tvae_pose_refine', 'classify_poses': 'tvae_pose_classify',
                              'polish_poses': 'tvae_pose_moments'}[name]
        assert cls.dtype == torch.int32 and cls.is_contiguous() and cls.reshape(-1).tolist() == [-1, 1, 2 ** 31 - 1], name
        seen.clear()


def test_pose_posteriors_shares_the_table_check(monkeypatch):
    from tvae import _cluster_lib as CL, ml2d
    from tvae._lib import TvaeHipError
    monkeypatch.setattr(CL, 'is_f32', lambda t, contiguous=True: True)
    num, yy, th, dx = torch.zeros(3, 1, 3, 3, 3), torch.zeros(3), torch.zeros(3), torch.zeros(3, 2)
    for cand in (torch.zeros(3, 1), torch.zeros(3, 1, dtype=torch.bool), torch.zeros(3, dtype=torch.int64)):
        with pytest.raises(TvaeHipError, match=r'^pose_posteriors: candidates must be an \[N\]\[M\] = \[3\]\[M\] integer array'):
            ml2d.pose_posteriors(num, num, yy, cand, th, dx, 8, 2, 1.0, angle_steps=1, shift=1)
    cand = torch.zeros(3, 1, dtype=torch.int64)
    for kw in (dict(angle_steps=33), dict(shift=9), dict(shift=-1), dict(t_scale=0.0), dict(angle_step=float('nan'))):
        kw = dict(dict(angle_steps=1, shift=1), **kw)
        A, S = kw['angle_steps'], kw['shift']
        tab = torch.zeros(3, 1, 2 * A + 1, abs(2 * S + 1), abs(2 * S + 1))
        with pytest.raises(TvaeHipError, match='^pose_posteriors: '):
            ml2d.pose_posteriors(tab, tab, yy, cand, th, dx, 8, 2, 1.0, **kw)


# ---- 4. the references of a round ---------------------------------------------------------------------------------------------------
def _fake_averages(monkeypatch, calls):
    """align.class_averages and align.class_halves replaced AFTER tvae.refine was imported: plane k of the averages holds k,
    plane (h, k) of the halves holds 100 (h + 1) + k."""
    from tvae import align

    def averages(im, th, dx, lab, K, t):
        calls.append(('averages', K, t))
        return torch.arange(K, dtype=torch.float32).reshape(K, 1, 1, 1).expand(K, 1, 4, 4).contiguous(), None

    def halves(im, th, dx, lab, K, t):
        calls.append(('halves', K, t))
        h = 100.0 * torch.arange(1, 3).reshape(2, 1) + torch.arange(K).reshape(1, K)
        return None, h.reshape(2, K, 1, 1, 1).expand(2, K, 1, 4, 4).contiguous(), None, None

    monkeypatch.setattr(align, 'class_averages', averages)
    monkeypatch.setattr(align, 'class_halves', halves)


def test_round_references(monkeypatch):
    from tvae import refine
    calls = []
    _fake_averages(monkeypatch, calls)
    Y, th, dx, lab = torch.zeros(6, 1, 4, 4), torch.zeros(6), torch.zeros(6, 2), torch.tensor([0, 1, 0, 0, 2, 1])
    refs = refine.round_references(Y, th, dx, lab, 3, 0.1, False)
    assert tuple(refs.shape) == (3, 1, 4, 4) and refs[:, 0, 0, 0].tolist() == [0, 1, 2] and calls == [('averages', 3, 0.1)]
    refs = refine.round_references(Y, th, dx, lab, 3, 1.0, True)
    assert tuple(refs.shape) == (6, 1, 4, 4) and refs[:, 0, 0, 0].tolist() == [100, 101, 102, 200, 201, 202]
    assert calls[1:] == [('halves', 3, 1.0)]


def test_every_rounds_function_takes_its_references_from_there(monkeypatch):
    from tvae import _cluster_lib as CL, classify, polish, refine
    monkeypatch.setattr(CL, 'is_f32', lambda t, contiguous=True: True)
    calls, seen = [], []
    _fake_averages(monkeypatch, calls)
    Y, th, dx, lab = torch.zeros(6, 1, 4, 4), torch.zeros(6), torch.zeros(6, 2), np.array([0, 1, 0, 0, 2, 1])

    def poses(images, theta, dx, labels, refs, *a, **kw):
        seen.append(refs[:, 0, 0, 0].tolist())
        N = images.shape[0]
        if torch.as_tensor(labels).dim() == 2:                # classify_poses
            M = labels.shape[1]
            return torch.as_tensor(labels)[:, 0].clone(), theta, dx, torch.zeros(N, M, 2), torch.zeros(N, 4, dtype=torch.int32)
        return theta, dx, torch.zeros(N, 2), torch.zeros(N, dtype=torch.int32)

    monkeypatch.setattr(refine, 'refine_poses', poses)
    monkeypatch.setattr(polish, 'polish_poses', poses)
    monkeypatch.setattr(classify, 'classify_poses', poses)
    for rounds in (refine.refine_rounds, polish.polish_rounds, classify.classify_rounds):
        for cross in (False, True):
            seen.clear()
            rounds(Y, th, dx, lab, 2, rounds=1, cross_halves=cross)
            assert seen == [[100, 101, 200, 201] if cross else [0, 1]], (rounds.__name__, cross)


# ---- 5. the resolution table ----------------------------------------------------------------------------------------------------------
def test_resolution_table(capsys):
    from tvae import stack_cli
    before = np.array([[8.0, 12.123456], [3.14159, 16.0]])
    after = np.array([[4.00004, 6.5], [2.99995, 16.0]])
    stack_cli.print_resolution_table(before, after, np.array([7, 0], dtype=np.int32))
    assert capsys.readouterr().out == ('# class  members  resolution[px]@0.143 before -> after  resolution[px]@0.5 before -> after\n'
                                       '0 7 8.0000 -> 4.0000 12.1235 -> 6.5000\n'
                                       '1 0 3.1416 -> 3.0000 16.0000 -> 16.0000\n')
    stack_cli.print_resolution_table(before, after, np.array([7, 0]), np.array([5.0, 2.0]))
    out, err = capsys.readouterr()
    assert out == ('# class  members before -> after  resolution[px]@0.143 before -> after  resolution[px]@0.5 before -> after\n'
                   '0 7 -> 5 8.0000 -> 4.0000 12.1235 -> 6.5000\n'
                   '1 0 -> 2 3.1416 -> 3.0000 16.0000 -> 16.0000\n') and err == ''


# ---- 6. the files of the four pose families ---------------------------------------------------------------------------------------------
FILES = {     # the module docstring of tvae/cluster_driver.py, family by family; .mrcs for particles, no .jpg without matplotlib
    'refine': ['rotations_refined.npy', 'translations_refined.npy', 'refine_scores.npy', 'class_averages_refined.npy'],
    'polish': ['rotations_polished.npy', 'translations_polished.npy', 'polish_scores.npy', 'polish_steps.npy',
               'class_averages_polished.npy'],
    'classify': ['clusters_reclassified.npy', 'rotations_reclassified.npy', 'translations_reclassified.npy', 'classify_scores.npy',
                 'classify_moved.npy', 'class_scores.npy', 'class_averages_reclassified.npy'],
    'ml2d': ['class_averages_ml.npy', 'class_weights.npy', 'clusters_ml.npy', 'rotations_ml.npy', 'translations_ml.npy',
             'ml_log_likelihood.npy', 'ml_sigma2.npy', 'ml_entropy.npy'],
}


@pytest.mark.parametrize('particles', [False, True])
def test_save_outputs_of_the_pose_families(tmp_path, monkeypatch, capsys, particles):
    from tvae import classify, figures, ml2d, polish, refine

    def no_plt():
        raise ImportError('no matplotlib here')

    monkeypatch.setattr(figures, '_plt', no_plt)
    N, K, M = 5, 2, 2
    th, d = torch.arange(N, dtype=torch.float32), torch.ones(N, 2)
    lab = torch.tensor([0, 1, 1, 0, 1])
    avg, counts = torch.zeros(K, 1, 6, 6), torch.tensor([2, 3], dtype=torch.int32)
    scores = np.zeros((1, 2))
    results = {
        'refine': (refine, (th, d, dict(scores=scores), avg, counts)),
        'polish': (polish, (th, d, dict(image_scores=np.zeros((N, 2), np.float32), image_steps=np.zeros(N, np.int32)), avg, counts)),
        'classify': (classify, (lab, th, d, dict(scores=scores, moved=np.zeros(1, np.int64), candidates=torch.zeros(N, M, dtype=torch.int64),
                                                 slot_scores=torch.zeros(N, M, 2)), avg, counts)),
        'ml2d': (ml2d, (avg, torch.ones(K, dtype=torch.float64), lab, th, d,
                        dict(log_likelihood=np.zeros(1), sigma2=np.ones(1), entropy=torch.zeros(N, dtype=torch.float64)))),
    }
    for family, (mod, result) in results.items():
        out = tmp_path / family
        out.mkdir()
        mod.save_outputs(str(out), *result, particles, (N, 1))
        want = FILES[family] + ([f for f in (x.replace('.npy', '.mrcs') for x in FILES[family] if x.startswith('class_averages_'))]
                                if particles else [])
        assert sorted(os.listdir(out)) == sorted(want), family
        rot = [f for f in want if f.startswith('rotations_')]
        assert len(rot) == 1 and np.load(out / rot[0]).shape == (N, 1) and np.load(out / rot[0]).dtype == np.float32
        assert np.array_equal(np.load(out / rot[0]).reshape(-1), th.numpy())
        assert np.load(out / rot[0].replace('rotations', 'translations')).shape == (N, 2)
        err = capsys.readouterr().err
        assert err.count('\n') == 1 and 'matplotlib is not available (no matplotlib here)' in err and '.jpg is skipped' in err
    assert np.load(tmp_path / 'classify' / 'class_scores.npy').shape == (N, K)
    assert np.load(tmp_path / 'ml2d' / 'clusters_ml.npy').tolist() == lab.tolist()


def test_the_driver_saves_the_polished_rotations_in_the_shape_of_the_run(tmp_path, monkeypatch, capsys):
    """TVAE_REFINE_POSES=1 hands its poses on to the polish as theta [N]; rotations_polished.npy still has the shape of the run's
    rotations, [N][1], as rotations_refined.npy has."""
    from tvae import align, cluster_driver, figures, polish
    import argparse

    def no_plt():
        raise ImportError('no matplotlib here')

    monkeypatch.setattr(figures, '_plt', no_plt)
    N = 4
    hist = dict(image_scores=np.zeros((N, 2), np.float32), image_steps=np.zeros(N, np.int32))
    monkeypatch.setattr(polish, 'polish_rounds', lambda y, th, d, lab, K, t: (th + 1, d, hist))
    monkeypatch.setattr(align, 'class_averages', lambda y, th, d, lab, K, t: (torch.zeros(K, 1, 6, 6), torch.zeros(K, dtype=torch.int32)))
    args = argparse.Namespace(n_clusters=2, t_inf='attention')
    run = (torch.zeros(N, 1, 6, 6), torch.device('cpu'), torch.zeros(N, 1), torch.zeros(N, 2), np.zeros(N, dtype=np.int64))
    for name, start in (('own', None), ('refined', (torch.full((N,), 5.0), torch.ones(N, 2)))):
        out = tmp_path / name
        out.mkdir()
        cluster_driver._polish_poses('particles', args, str(out), *run, start=start)
        rot = np.load(out / 'rotations_polished.npy')
        assert rot.shape == (N, 1) and rot.reshape(-1).tolist() == [1.0 if start is None else 6.0] * N
        assert (out / 'class_averages_polished.mrcs').exists()
    with pytest.raises(SystemExit, match='^TVAE_POLISH_POSES=1 needs square images, these are 6 x 5$'):
        cluster_driver._polish_poses('particles', args, str(tmp_path), torch.zeros(N, 1, 6, 5), *run[1:])
    assert capsys.readouterr().err.count('# polishing the poses against the class averages ... \n') == 3


if __name__ == '__main__' and sys.argv[1:] == ['--record']:
    with open(PARSERS_JSON, 'w') as f:
        json.dump({k: _snapshot(p) for k, p in _parsers().items()}, f, indent=1, sort_keys=True)
        f.write('\n')
