"""Particle preprocessing, the part that needs no GPU: the fp64 restatement tests/image_ref.py and the table form of
tvae.tables.resample_tables against the goldens of the reference's src/image.py (tests/golden/image_ref.npz), the tables'
structure and cache, the header against the binding for the new names, the host query of libtvae_cluster.so, the command
line's parser and the refusal of CPU tensors."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import image_ref
from conftest import PKG, ROOT, load_golden

N_DOWN, N_NORM = 10, 4


@pytest.fixture(scope='module')
def gold():
    return load_golden('image_ref')


def _tol(x):
    return 1e-12 * np.abs(x).max()


# ---- restatement and tables against the reference's results ----------------------------------------------------------------
def test_golden_file_is_small_and_complete(gold):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'image_ref.npz')) < 100 * 1024
    shapes = [(gold[f'down{k}_x'].shape[1:], tuple(gold[f'down{k}_shape'])) for k in range(N_DOWN)]
    assert shapes == [((16, 16), (8, 8)), ((16, 16), (7, 7)), ((15, 15), (6, 6)), ((15, 17), (5, 8)), ((20, 24), (7, 10)),
                      ((8, 8), (1, 1)), ((8, 8), (3, 2)), ((12, 10), (12, 10)), ((13, 11), (13, 11)), ((9, 6), (4, 6))]
    assert [gold[f'norm{k}_x'].shape[1:] for k in range(N_NORM)] == [(7, 9), (7, 9), (16, 16), (16, 16)]
    assert all(v.dtype == np.float64 for k, v in gold.items() if k.endswith(('_x', '_y')))


@pytest.mark.parametrize('k', range(N_DOWN))
def test_downsample_restatement_and_tables(gold, k):
    from tvae import tables
    x, want = gold[f'down{k}_x'], gold[f'down{k}_y']
    m, n = (int(v) for v in gold[f'down{k}_shape'])
    M, N = x.shape[-2:]
    assert want.shape == (1, m, n)
    assert np.abs(image_ref.downsample(x, (m, n)) - want).max() <= _tol(x)
    Ar, Ai, Br, Bi = tables.resample_tables_f64(M, N, m, n)
    assert Ar.shape == Ai.shape == (m, M) and Br.shape == Bi.shape == (N, n)
    assert np.abs(image_ref.sandwich(x, Ar, Ai, Br, Bi, 1.0 / (M * N)) - want).max() <= _tol(x)
    # the tables are the parts of the complex matrices of the definition, summed independently here
    Ry, Kx = image_ref.complex_tables(M, N, m, n)
    assert np.abs(Ar - Ry.real).max() <= 1e-12 * m and np.abs(Ai - Ry.imag).max() <= 1e-12 * m
    assert np.abs(Br - Kx.real).max() <= 1e-12 * n and np.abs(Bi - Kx.imag).max() <= 1e-12 * n


def test_downsample_by_a_factor(gold):
    from tvae import image
    x, want = gold['downf_x'], gold['downf_y']
    m, n = image.output_shape(16, 12, float(gold['downf_factor']))
    assert (m, n) == (6, 4) == want.shape[1:] and image.output_shape(16, 12, shape=(5, 3)) == (5, 3)
    assert image.output_shape(100, 100, 3) == (33, 33) and image.output_shape(7, 9) == (7, 9)
    assert np.abs(image_ref.downsample(x, (m, n)) - want).max() <= _tol(x)


def test_table_structure():
    from tvae import tables
    assert tables.resample_source_rows(16, 7).tolist() == [0, 1, 2, 12, 13, 14, 15]      # the last ceil(7 / 2) rows
    assert tables.resample_source_rows(16, 8).tolist() == [0, 1, 2, 3, 12, 13, 14, 15]
    assert tables.resample_source_rows(8, 1).tolist() == [7] and image_ref.source_rows(16, 7) == [0, 1, 2, 12, 13, 14, 15]
    for M in (12, 13):
        Ry, Kx = image_ref.complex_tables(M, M, M, M)
        assert np.abs(Ry.imag).max() <= 1e-12 * M and np.abs(Ry.real - M * np.eye(M)).max() <= 1e-12 * M     # Im Ry vanishes at m = M
        assert np.abs(Kx.real - M * np.eye(M)).max() <= 1e-12 * M
        Ar, Ai, Br, Bi = tables.resample_tables_f64(M, M, M, M)
        assert not Ai.any() and np.abs(Ar - M * np.eye(M)).max() <= 1e-12 * M
    # rank of Im Ry: 1 for even m < M, 2 for odd m < M
    for (M, m), rank in (((16, 8), 1), ((16, 7), 2), ((15, 6), 1), ((15, 5), 2)):
        s = np.linalg.svd(tables.resample_tables_f64(M, M, m, m)[1], compute_uv=False)
        assert (s > 1e-9 * s[0]).sum() == rank, (M, m, s[:4])
    with pytest.raises(ValueError):
        tables.resample_tables_f64(8, 8, 9, 4)
    with pytest.raises(ValueError):
        tables.resample_tables_f64(8, 8, 4, 0)


def test_table_cache_is_keyed_by_shape():
    from tvae import tables
    a = tables.resample_tables(20, 24, 7, 10)
    assert tables.resample_tables(20, 24, 7, 10) is a and tables.resample_tables_f64(20, 24, 7, 10) is tables.resample_tables_f64(20, 24, 7, 10)
    b = tables.resample_tables(24, 20, 7, 10)
    assert b is not a and [t.shape for t in b] == [(7, 24), (7, 24), (20, 10), (20, 10)]
    assert [t.shape for t in a] == [(7, 20), (7, 20), (24, 10), (24, 10)]
    assert all(t.dtype == np.float32 and t.flags.c_contiguous and not t.flags.writeable for t in a)
    for t32, t64 in zip(a, tables.resample_tables_f64(20, 24, 7, 10)):
        assert np.array_equal(t32, t64.astype(np.float32))                 # rounded once


@pytest.mark.parametrize('k', range(N_NORM))
def test_normalize_restatement(gold, k):
    x, want, radius = gold[f'norm{k}_x'], gold[f'norm{k}_y'], float(gold[f'norm{k}_radius'])
    got, stats = image_ref.normalize(x, None if np.isnan(radius) else radius)
    assert np.abs(got - want).max() <= _tol(x)
    assert np.abs(stats[:, 0] - 1000).max() < 2 and np.abs(stats[:, 1] - 1).max() < 0.5


def test_normalize_degenerate_cases(gold):
    got, stats = image_ref.normalize(gold['norm_empty_x'], float(gold['norm_empty_radius']))
    assert np.isnan(gold['norm_empty_y']).all() and np.isnan(got).all() and np.isnan(stats).all()
    got, stats = image_ref.normalize(gold['norm_const_x'])
    want = gold['norm_const_y']
    assert not np.isfinite(want).any() and (stats[:, 1] == 0).all() and (stats[:, 0] == 2.5).all()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    # the centre is (n / 2, m / 2): for 8 x 8 the pixel (0, 4) is at distance exactly 4 and belongs to the default ring
    mask = image_ref.ring_mask(8, 8)
    assert mask[0, 4] and mask[4, 0] and not mask[1, 4] and not mask[7, 4] and mask[0, 0]
    assert np.array_equal(mask, np.hypot(4.0 - np.arange(8)[:, None], 4.0 - np.arange(8)[None, :]) >= 4.0)


def test_crop(gold):
    from tvae import image
    x, want = gold['crop_x'], gold['crop_y']
    assert np.array_equal(image_ref.crop(x, int(gold['crop_size'])), want)
    t = torch.from_numpy(x)
    got = image.crop(t, 4)
    assert np.array_equal(got.numpy(), want) and got.data_ptr() == t[0, 2:, 3:].data_ptr()      # a view, no copy
    assert image.crop_window(9, 10, 4) == (2, 3)
    import src.image as drop_in
    assert np.array_equal(drop_in.crop(x, 4), want) and np.shares_memory(drop_in.crop(x, 4), x)


# ---- header, binding, queries ----------------------------------------------------------------------------------------------
NEW_CALLS = {'tvae_image_resample': 'pppppp' 'iiiiiiiii' 'f', 'tvae_image_normalize': 'ppppliiif'}
NEW_QUERIES = {'tvae_image_normalize_ws_floats': ('iii', 'l')}


def test_header_and_binding_of_the_new_entry_points():
    from tvae import _cluster_lib as CL, _lib
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
    for name, sig in NEW_CALLS.items():
        assert CL.SIGNATURES[name] == sig
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[-1].startswith('tvae_stream_t') and len(args) - 1 == len(sig)
        for a, c in zip(args[:-1], sig):
            assert ('*' in a) == (c == 'p') and a.startswith({'p': ('const ', 'float', 'int', 'double'), 'f': 'float ',
                                                               'l': 'long ', 'i': 'int '}[c]), (name, a)
    for name, (sig, ret) in NEW_QUERIES.items():
        assert CL.QUERIES[name] == (sig, ret)
        m = re.search(r'\b(int|long)\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m and m.group(1) == {'i': 'int', 'l': 'long'}[ret]
        assert all(a.strip().startswith('int ') for a in m.group(2).split(',')) and len(m.group(2).split(',')) == len(sig)
    assert re.search(r'double\*\s+stats', hdr) and ('tvae_image_normalize', 2) in _lib._F64_OK
    L = CL.lib()
    assert L.tvae_cluster_abi_version() == CL.ABI_VERSION == 1
    for name in list(NEW_CALLS) + list(NEW_QUERIES):
        assert hasattr(L, name), name
    flat = ' '.join(hdr.split())
    assert 'GENERIC batched sandwich product' in flat and "reference's slicing rule" in flat and 'TWO passes' in flat


def test_query():
    from tvae import _cluster_lib as CL
    for B, n, m in [(1, 1, 1), (3, 7, 9), (5, 64, 64), (2, 130, 70), (100000, 64, 64), (1 << 24, 64, 64), (7, 1024, 1024)]:
        assert CL.query('tvae_image_normalize_ws_floats', B, n, m) == 6 * B * -(-n * m // 4096), (B, n, m)
    for bad in [(0, 8, 8), (-1, 8, 8), ((1 << 24) + 1, 8, 8), (4, 0, 8), (4, 8, 0), (4, 1025, 8), (4, 8, 1025), (4, -3, 8),
                (1 << 24, 1024, 1024)]:                                   # the last one: 2^32 workgroups
        assert CL.query('tvae_image_normalize_ws_floats', *bad) == 0, bad


# ---- command line and host side --------------------------------------------------------------------------------------------
def _flags(parser):
    return sorted(s for a in parser._actions for s in a.option_strings if s not in ('-h', '--help'))


def test_preprocess_particles_parser():
    from tvae import image
    p = image.build_parser()
    assert _flags(p) == sorted(['--stack', '--out', '--crop', '--downsample', '--shape', '--normalize', '--radius', '--chunk', '-d'])
    a = p.parse_args(['--stack', 's.mrcs', '--out', 'o.mrcs'])
    assert (a.crop, a.downsample, a.shape, a.normalize, a.radius, a.chunk, a.device) == (0, 1, None, False, None, 4096, 0)
    a = p.parse_args(['--stack', 's.mrcs', '--out', 'o.mrcs', '--crop', '200', '--shape', '64', '48', '--normalize', '--radius',
                      '20.5', '--chunk', '512', '-d', '1'])
    assert (a.crop, a.shape, a.normalize, a.radius, a.chunk, a.device) == (200, [64, 48], True, 20.5, 512, 1)
    assert p.parse_args(['--stack', 's', '--out', 'o', '--downsample', '2.5']).downsample == 2.5
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's', '--out', 'o', '--downsample', '2', '--shape', '8', '8'])
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's.mrcs'])
    spec = importlib.util.spec_from_file_location('preprocess_particles_script', os.path.join(PKG, 'preprocess_particles.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run is image.run and callable(mod.main)


def test_image_bench_parser_and_flop_count():
    spec = importlib.util.spec_from_file_location('image_bench', os.path.join(ROOT, 'profiles', 'tools', 'image_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert _flags(p) == sorted(['--shapes', '--images', '--chunk', '--host-images', '--reps', '--warmup', '--tag', '--out'])
    a = p.parse_args([])
    assert a.shapes == ['256-64', '256-128', '128-64'] and a.images == [20000, 100000] and (a.reps, a.warmup) == (10, 2)
    assert mod.parse_shape('256-64') == (256, 64)
    # 256^2 -> 64^2, one 64 x 64 tile, four chunks: 2 (Ar, Ai) * 2 * 64 * 256 * 256 for stage 1 and 2 * 2 * 64 * 256 * 64 for stage 2
    assert mod.issued_flop(1, 256, 256, 64, 64, True) == 2 * 2 * 64 * 256 * 256 + 2 * 2 * 64 * 256 * 64
    assert mod.issued_flop(3, 256, 256, 64, 64, False) == 3 * (2 * 64 * 256 * 256 + 2 * 64 * 256 * 64)
    # its two baselines are the reference's route
    gold = load_golden('image_ref')
    for k in range(N_DOWN):
        x, s = gold[f'down{k}_x'], tuple(int(v) for v in gold[f'down{k}_shape'])
        assert np.abs(mod.numpy_route(x, *s) - gold[f'down{k}_y']).max() <= _tol(x)
        assert np.abs(mod.fft_route(torch.from_numpy(x), *s).numpy() - gold[f'down{k}_y']).max() <= _tol(x)


def test_drop_in_has_the_reference_signatures():
    import inspect
    import src.image as drop_in
    assert str(inspect.signature(drop_in.downsample)) == '(x, factor=1, shape=None)'
    assert str(inspect.signature(drop_in.crop)) == '(stack, size)'
    assert str(inspect.signature(drop_in.normalize)) == '(stack, radius=None)'


def test_cpu_tensors_are_refused():
    from tvae import image
    x = torch.zeros(2, 8, 8)
    with pytest.raises(image.TvaeHipError):
        image.downsample(x, 2)
    with pytest.raises(image.TvaeHipError):
        image.normalize(x)
