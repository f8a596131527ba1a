"""Half sets, variance maps and the ring correlation of the class averages, the part that needs no GPU: the fp64
restatement tests/frc_ref.py against an independent direct DFT and against the float ring rule, the mask, the host-only
tvae.resolution.resolution, the new parser and bench parser, the header against the binding for the new names, the host
queries of libtvae_cluster.so and the refusal of CPU tensors."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import frc_ref
from conftest import PKG, ROOT


# ---- the restatement -------------------------------------------------------------------------------------------------------
def direct_frc(a, b, m):
    """O(n^4): every coefficient as the plain double sum, rings by the integer inequality itself."""
    n = a.shape[0]
    k = frc_ref.signed_freq(n)
    R = n // 2 + 1
    sums = np.zeros((R, 3))
    for yi, ky in enumerate(k):
        for xi, kx in enumerate(k):
            fa = fb = 0j
            for i in range(n):
                for j in range(n):
                    w = np.exp(-2j * np.pi * ((ky * i + kx * j) % n) / n)
                    fa += a[i, j] * m[i, j] * w
                    fb += b[i, j] * m[i, j] * w
            s4 = 4 * (int(ky) ** 2 + int(kx) ** 2)
            r = [r for r in range(2 * n) if (r == 0 or (2 * r - 1) ** 2 <= s4) and s4 < (2 * r + 1) ** 2]
            assert len(r) == 1
            if r[0] < R:
                sums[r[0]] += [(fa * np.conj(fb)).real, abs(fa) ** 2, abs(fb) ** 2]
    return sums


@pytest.mark.parametrize('n', [5, 6])
def test_restatement_against_a_direct_dft(n):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal((2, n, n))
    for radius, edge in ((None, 0.0), (0.35 * n, 1.5)):
        ref = frc_ref.frc(a[None], b[None], radius, edge)
        want = direct_frc(a, b, frc_ref.mask(n, radius, edge))
        assert ref['sums'].shape == (1, n // 2 + 1, 3)
        assert np.abs(ref['sums'][0] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(ref['frc'][0] - want[:, 0] / np.sqrt(want[:, 1] * want[:, 2])).max() <= 1e-12


@pytest.mark.parametrize('n', [5, 6, 16, 33])
def test_ring_rule_against_the_rounded_radius(n):
    k = frc_ref.signed_freq(n)
    assert sorted(k.tolist()) == list(range(-(n // 2), (n + 1) // 2))
    assert np.array_equal(k, np.round(np.fft.fftfreq(n) * n).astype(int))
    ring = frc_ref.ring_index(n)
    want = np.floor(np.hypot(k[:, None].astype(np.float64), k[None, :].astype(np.float64)) + 0.5).astype(int)
    assert np.array_equal(ring, want)
    assert ring[0, 0] == 0 and (ring == 0).sum() == 1 and set(range(n // 2 + 1)) <= set(ring.reshape(-1).tolist())


@pytest.mark.parametrize('n', [16, 33])
def test_a_single_cosine_sits_in_ring_five(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    a = np.cos(2 * np.pi * (3 * i + 4 * j) / n)
    ref = frc_ref.frc(a[None], a[None])
    power = ref['sums'][0, :, 1]
    assert abs(power[5] - n ** 4 / 2) <= 1e-9 * n ** 4                   # two coefficients of n^2 / 2 each
    assert np.abs(np.delete(power, 5)).max() <= 1e-18 * n ** 4
    assert abs(ref['frc'][0, 5] - 1) <= 1e-12


def test_mask_regimes():
    n, radius, edge = 33, 10.0, 4.0
    m = frc_ref.mask(n, radius, edge)
    c = (n - 1) / 2
    i, j = np.meshgrid(np.arange(n) - c, np.arange(n) - c, indexing='ij')
    d = np.hypot(i, j)
    assert (m[d <= radius] == 1).all() and (m[d >= radius + edge] == 0).all()
    soft = (d > radius) & (d < radius + edge)
    assert soft.sum() > 100 and ((m[soft] > 0) & (m[soft] < 1)).all()
    assert np.allclose(m[soft], 0.5 * (1 + np.cos(np.pi * (d[soft] - radius) / edge)), rtol=0, atol=1e-15)
    assert abs(m[16, 16 + 12] - 0.5) <= 1e-15                            # half way down the edge
    assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1])
    hard = frc_ref.mask(n, radius, 0.0)
    assert set(np.unique(hard)) == {0.0, 1.0} and np.array_equal(hard == 1, d <= radius)
    for none in (None, 0.0, -3.0):
        assert (frc_ref.mask(n, none, edge) == 1).all()


def test_half_lists_keep_the_position_parity():
    order = np.array([7, -1, 3, 99, 5, 2, 8, 4])
    seg = np.array([0, 5, 5, 8])
    lists = frc_ref.half_lists(order, seg, 10)
    assert [[m.tolist() for m in pair] for pair in lists] == [[[7, 3, 5], []], [[], []], [[2, 4], [8]]]
    A = np.arange(10.0).reshape(10, 1, 1, 1) * np.ones((1, 1, 2, 2))
    avg, halves, var, counts = frc_ref.class_halves(A, order, seg)
    assert counts.tolist() == [[3, 0], [0, 0], [2, 1]]
    assert avg[:, 0, 0, 0].tolist() == [5.0, 0.0, 14 / 3] and halves[:, :, 0, 0, 0].tolist() == [[5.0, 0.0, 3.0], [0.0, 0.0, 8.0]]
    assert np.allclose(var[:, 0, 0, 0], [4.0, 0.0, np.var([2, 8, 4], ddof=1)])


# ---- resolution ------------------------------------------------------------------------------------------------------------
def test_resolution():
    from tvae.resolution import resolution
    n = 16                                                               # R = 9
    curve = np.array([1.0, 0.9, 0.8, 0.6, 0.4, 0.2, 0.1, 0.05, 0.0])
    assert resolution(curve, n, 0.4) == pytest.approx(n / 4.0, rel=1e-15)      # ring 4 equals the threshold: not below it ...
    assert resolution(curve, n, 0.4) == n / (4 + (0.4 - 0.4) / 0.2)            # ... the crossing is at ring 4 exactly
    assert resolution(curve, n, 0.5) == pytest.approx(n / 3.5, rel=1e-15)      # half way between rings 3 and 4
    assert resolution(curve, n, 0.143) == pytest.approx(n / (5 + (0.2 - 0.143) / 0.1), rel=1e-15)
    assert resolution(curve, n) == resolution(curve, n, 0.143)
    assert resolution(np.full(9, 0.9), n, 0.5) == n / 8                        # never crosses: the last ring
    assert resolution(np.array([1.0, 0.1] + [0.9] * 7), n, 0.5) == n / 1.0     # crossing inside the first ring: r* >= 1
    assert resolution(np.array([0.0, 0.0] + [0.9] * 7), n, 0.5) == n / 1.0     # ring 0 below it as well
    assert resolution(curve, n, 0.5, apix=1.5) == pytest.approx(1.5 * n / 3.5, rel=1e-15)
    # odd n: the same nine rings belong to n = 17, which is why n is an argument
    assert resolution(curve, 17, 0.5) == pytest.approx(17 / 3.5, rel=1e-15)
    both = resolution(np.stack([curve, np.full(9, 0.9)])[None], n, 0.5)
    assert both.shape == (1, 2) and both[0].tolist() == [resolution(curve, n, 0.5), n / 8]
    with pytest.raises(ValueError):
        resolution(curve, 20)


def test_combined_curve():
    from tvae import resolution
    rng = np.random.default_rng(2)
    s = rng.uniform(0.5, 2.0, (3, 2, 5, 3))
    s[1, :, 2, 1] = 0.0
    c = resolution.combined(s)
    t = s.sum(1)
    assert c.shape == (3, 5) and c[1, 2] == 0.0
    assert np.allclose(c[0], t[0, :, 0] / np.sqrt(t[0, :, 1] * t[0, :, 2]), rtol=1e-15)
    assert resolution.default_mask(65) == (28.0, 4.0) and resolution.default_mask(65, 10, 0) == (10.0, 0.0)
    assert 'gold-standard' in resolution.NOTE and 'optimistic' in resolution.NOTE


# ---- parsers ---------------------------------------------------------------------------------------------------------------
def _flags(parser):
    return sorted(s for a in parser._actions for s in a.option_strings if s not in ('-h', '--help'))


def test_class_resolution_parser():
    from tvae import resolution
    p = resolution.build_parser()
    assert _flags(p) == sorted(['--stack', '--rotations', '--translations', '--clusters', '--t-inf', '--crop', '--n-clusters',
                                '--out-dir', '-d', '--device', '--apix', '--threshold', '--mask-radius', '--mask-edge'])
    need = ['--stack', 's.mrcs', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy']
    a = p.parse_args(need)
    assert (a.t_inf, a.crop, a.n_clusters, a.out_dir, a.device) == ('attention', 0, None, '.', 0)
    assert (a.apix, a.threshold, a.mask_radius, a.mask_edge) == (None, 0.143, None, 4.0)
    a = p.parse_args(need + ['--apix', '1.2', '--threshold', '0.5', '--mask-radius', '20', '--mask-edge', '0', '-d', '1',
                             '--t-inf', 'unimodal', '--crop', '40', '--n-clusters', '7', '--out-dir', 'o'])
    assert (a.apix, a.threshold, a.mask_radius, a.mask_edge, a.device) == (1.2, 0.5, 20.0, 0.0, 1)
    assert (a.t_inf, a.crop, a.n_clusters, a.out_dir) == ('unimodal', 40, 7, 'o')
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's.npy'])
    spec = importlib.util.spec_from_file_location('class_resolution_script', os.path.join(PKG, 'class_resolution.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run is resolution.run and callable(mod.main)


def test_existing_parsers_are_unchanged():
    from tvae import align, cluster_driver
    assert _flags(align.build_parser()) == sorted(['--stack', '--rotations', '--translations', '--clusters', '--t-inf', '--crop',
                                                   '--n-clusters', '--out-dir', '--write-aligned', '-d', '--device'])
    for kind in ('mnist', 'dsprites', 'galaxy', 'particles'):
        flags = _flags(cluster_driver.build_parser(kind))
        assert not [f for f in flags if 'frc' in f or 'resol' in f or 'half' in f or 'mask' in f or 'apix' in f], kind


def test_class_stats_bench_parser():
    spec = importlib.util.spec_from_file_location('class_stats_bench',
                                                  os.path.join(ROOT, 'profiles', 'tools', 'class_stats_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert _flags(p) == sorted(['--shapes', '--clusters', '--channels', '--frc-planes', '--frc-sides', '--reps', '--warmup',
                                '--out', '--skip-route', '--tag'])
    a = p.parse_args([])
    assert a.shapes == ['20000x64', '100000x128'] and a.clusters == [10] and a.channels == 1
    assert a.frc_planes == 100 and a.frc_sides == [128, 256] and a.reps == 10
    assert mod.parse_shape('20000x64') == (20000, 64)


# ---- header, binding, queries ----------------------------------------------------------------------------------------------
NEW_CALLS = {'tvae_class_halves': 'pppppppppp' 'l' 'iiiif', 'tvae_class_frc': 'pppppliiff'}
NEW_QUERIES = {'tvae_class_halves_ws_floats': ('iiii', 'l'), 'tvae_frc_rings': ('i', 'i'),
               'tvae_class_frc_ws_floats': ('ii', 'l')}


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
    assert re.search(r'double\*\s+sums', hdr) and ('tvae_class_frc', 3) in _lib._F64_OK
    assert int(re.search(r'#define\s+TVAE_FRC_MAX_PLANES\s+(\d+)', hdr).group(1)) == 65535
    L = CL.lib()
    assert L.tvae_cluster_abi_version() == 1
    for name in list(NEW_CALLS) + list(NEW_QUERIES):
        assert hasattr(L, name), name
    # the header says what the issue asks it to say
    flat = ' '.join(hdr.split())
    assert 'NOT bit for bit' in flat and 'relative to Q / m' in flat


def test_queries():
    from tvae import _cluster_lib as CL
    for n in (2, 5, 6, 33, 64, 65, 1023, 1024):
        assert CL.query('tvae_frc_rings', n) == n // 2 + 1
        for P in (1, 24, 65535):
            assert CL.query('tvae_class_frc_ws_floats', P, n) == P * 7 * n * (n // 2 + 1)
    for n in (-5, 0, 1, 1025, 1 << 20):
        assert CL.query('tvae_frc_rings', n) == 0 and CL.query('tvae_class_frc_ws_floats', 3, n) == 0
    for P in (0, -1, 65536):
        assert CL.query('tvae_class_frc_ws_floats', P, 16) == 0
    for N, K, C, n in [(400, 5, 3, 33), (20000, 100, 1, 64), (100000, 10, 1, 128), (1, 1, 1, 2), (7, 3, 2, 1024)]:
        chunk = CL.query('tvae_class_average_chunk', N, K, C, n)
        slots = N // chunk + K
        ints = (K + 1 + 2 * slots + 3) // 4 * 4
        assert CL.query('tvae_class_halves_ws_floats', N, K, C, n) == ints + 3 * slots * C * n * n
    for bad in [(400, 5, 1, 1), (400, 5, 1, 1025), (400, 0, 1, 16), (400, 5, 0, 16), (0, 5, 1, 16), (-1, 5, 1, 16),
                (400, 65536, 1, 16), (400, 5, 1025, 16), ((1 << 24) + 1, 5, 1, 16), (1 << 24, 5, 64, 1024)]:
        assert CL.query('tvae_class_halves_ws_floats', *bad) == 0, bad
    # the slot count tripled where it bounds the grid: (N / 32 + K) C tiles is within 2^31 here, three times it is not
    N, K, C, n = 100000, 65535, 4, 1024
    assert CL.query('tvae_class_average_ws_floats', N, K, C, n) > 0 and CL.query('tvae_class_halves_ws_floats', N, K, C, n) == 0


def test_cpu_tensors_are_refused():
    from tvae import align
    y, th, dx = torch.zeros(4, 1, 8, 8), torch.zeros(4), torch.zeros(4, 2)
    with pytest.raises(align.TvaeHipError):
        align.class_halves(y, th, dx, torch.zeros(4, dtype=torch.int64), 2)
    with pytest.raises(align.TvaeHipError):
        align.frc(y, y)
    with pytest.raises(align.TvaeHipError):
        align.frc(y[0, 0], y[0, 0], 3.0, 1.0)
