"""The host side of the CTF correction without a GPU: tvae.ctf.coefficients and the fp64 restatement tests/ctf_ref.py against
the reference's own arithmetic (src/ctf.py) and its own filters (tests/golden/ctf_filters.npz), the sign rule, the float32
restatement and the a-priori bound that test_ctf_gpu.py measures the kernel with, the command lines' new flags, and the
header against the binding."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import ctf_ref
from conftest import PKG, ROOT, load_golden, rel_err

COLS = ['defocus', 'cs', 'voltage', 'apix', 'bfactor', 'ampcont', 'dfdiff', 'dfang']


def _golden_table():
    fx = load_golden('ctf_filters')
    return fx, np.stack([fx[c] for c in COLS], 1).astype(np.float64), int(fx['n'])


@pytest.mark.parametrize('n', (31, 32))
@pytest.mark.parametrize('scale', (1, 2))
def test_coefficients_restate_compute_2d_ctf(n, scale):
    import src.ctf as C
    from tvae import ctf
    _, tab, _ = _golden_table()
    rng = np.random.default_rng(n)
    more = np.stack([rng.uniform(1, 3, 6), np.full(6, 2.7), np.full(6, 300.0), np.full(6, 1.2), rng.uniform(50, 150, 6),
                     rng.uniform(5, 12, 6), rng.uniform(0, 0.2, 6), rng.uniform(0, 180, 6)], 1)
    tab = np.concatenate([tab, more])
    f = np.fft.fftfreq(n)
    gy, gx = np.meshgrid(f, f[:n // 2 + 1], indexing='ij')
    freqs = np.stack([gy.ravel(), gx.ravel()], 1)
    for sign in (1, -1):
        coef = ctf.coefficients(tab, scale=scale, sign=sign)
        assert coef.shape == (len(tab), 5) and coef.dtype == np.float64
        got = ctf_ref.H(coef, n)
        for i, row in enumerate(tab):
            apix = row[3] * scale
            want = C.compute_2d_ctf(freqs / apix, row[0] * 10000, row[0] * 10000, 2 * np.pi * row[7] / 360, row[2], row[1],
                                    row[5] / 100, row[4]).reshape(n, n // 2 + 1)
            assert np.abs(got[i] - sign * want).max() <= 1e-12, (i, sign)
    # a DataFrame and a mapping give the same rows; the default is the model's sign
    import pandas as pd
    frame = pd.DataFrame({c: tab[:, k] for k, c in enumerate(COLS)})
    assert np.array_equal(ctf.coefficients(frame, scale), ctf.coefficients(tab, scale, -1))
    assert np.array_equal(ctf.coefficients({c: tab[:, k] for k, c in enumerate(COLS)}, scale), ctf.coefficients(tab, scale))
    with pytest.raises(ValueError):
        ctf.coefficients(tab, sign=0)
    with pytest.raises(ValueError):
        ctf.coefficients(tab[:, :5])


def test_reference_filter_of_the_centred_delta_is_the_golden_filter_bank():
    from tvae import ctf
    fx, tab, n = _golden_table()
    delta = np.zeros((n, n))
    delta[n // 2, n // 2] = 1.0
    got = ctf_ref.filter(delta[None], ctf_ref.H(ctf.coefficients(tab), n))
    assert got.shape == fx['filters'].shape and rel_err(got, fx['filters']) < 1e-6
    # an even size against src.ctf itself: -fftshift(Re ifft2(c)) puts the origin at n // 2 as well
    import pandas as pd
    import src.ctf as C
    host = C.ctf_filter(pd.DataFrame({c: fx[c] for c in COLS}), 32, 32)
    d32 = np.zeros((32, 32))
    d32[16, 16] = 1.0
    assert rel_err(ctf_ref.filter(d32[None], ctf_ref.H(ctf.coefficients(tab), 32)), host) < 1e-6


def test_sign_rule_and_half_plane_conventions():
    coef = np.array([[0.0, 0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 3.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0, 0.0]])
    s = ctf_ref.H(coef, 8, 1)
    assert (s[0] == 1).all()                                             # H = 0 everywhere: +1
    v = ctf_ref.H(coef, 8)
    assert np.array_equal(s[1], np.where(v[1] < 0, -1.0, 1.0)) and (s[1] == -1).any() and (s[1] == 1).any()
    assert (s[2] == -1).all()
    assert list(ctf_ref.signed(5)) == [0, 1, 2, -2, -1] and list(ctf_ref.signed(4)) == [0, 1, -2, -1]
    assert list(ctf_ref.weights(4)) == [1, 2, 1] and list(ctf_ref.weights(5)) == [1, 2, 2]
    assert ctf_ref.q_grid(4)[2, 2] == 8 / 16 and ctf_ref.q_grid(5)[3, 1] == 5 / 25
    # the filter of the definition (half-spectrum sum with weights) is the full-plane product with H(-ky, -kx)
    rng = np.random.default_rng(3)
    for n in (4, 5):
        R = n // 2 + 1
        x, Hh = rng.standard_normal((n, n)), rng.standard_normal((n, R))
        X = np.fft.fft2(x)
        i, j = np.mgrid[:n, :n]
        want = np.zeros((n, n))
        for ky in range(n):
            for kx in range(R):
                want += ctf_ref.weights(n)[kx] * (Hh[ky, kx] * X[ky, kx] * np.exp(2j * np.pi * (ky * i + kx * j) / n)).real
        assert np.abs(ctf_ref.filter(x[None], Hh)[0] - want / n ** 2).max() < 1e-12


@pytest.mark.parametrize('n', (2, 3, 8, 33))
def test_float32_restatement_and_bound(n):
    """filter_f32 is the same four stages (it agrees with fp64 to float32 rounding) and filter_bound really bounds it."""
    rng = np.random.default_rng(50 + n)
    x = (rng.standard_normal((3, n, n)) + 0.5).astype(np.float32)
    Hh = rng.standard_normal((3, n, n // 2 + 1)).astype(np.float32)
    ref = ctf_ref.filter(x, Hh.astype(np.float64))
    got = ctf_ref.filter_f32(x, Hh)
    assert got.dtype == np.float32
    err = np.sqrt(((got - ref) ** 2).sum((1, 2)))
    bound = ctf_ref.filter_bound(x, Hh.astype(np.float64))
    assert (err <= bound).all() and (bound <= 1e-3 * np.sqrt((ref ** 2).sum((1, 2)))).all()
    assert np.abs(ctf_ref.filter_f32(x, np.ones((n, n // 2 + 1), np.float32)) - x).max() <= 64 * 2.0 ** -24 * np.abs(x).max()


def test_power_reference_follows_the_order_and_seg_rules():
    rng = np.random.default_rng(4)
    coef = np.column_stack([rng.standard_normal((6, 2)), rng.uniform(-50, 50, (6, 2)), rng.uniform(0, 5, 6)])
    order, seg = np.array([4, -1, 0, 9, 2, 5]), np.array([0, 3, 1, 99])
    D, counts = ctf_ref.power(coef, order, seg, 5)
    h2 = ctf_ref.H(coef, 5) ** 2
    assert list(counts) == [2, 0, 2] and (D[1] == 0).all()
    assert np.allclose(D[0], h2[4] + h2[0]) and np.allclose(D[2], h2[2] + h2[5])


# ---- command lines ---------------------------------------------------------------------------------------------------------
def _flags(parser):
    return sorted(s for a in parser._actions for s in a.option_strings if s not in ('-h', '--help'))


def test_parsers_gain_the_ctf_flags():
    from tvae import align, resolution
    need = ['--stack', 's.mrcs', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy']
    p = align.build_parser(ctf=True)
    assert sorted(set(_flags(p)) - set(_flags(align.build_parser()))) == ['--ctf', '--ctf-correct', '--scale', '--wiener-tau']
    a = p.parse_args(need)
    assert (a.ctf, a.ctf_correct, a.wiener_tau, a.scale) == (None, 'wiener', 0.1, 1)
    a = p.parse_args(need + ['--ctf', 'c.txt', '--ctf-correct', 'flip', '--wiener-tau', '0.02', '--scale', '2'])
    assert (a.ctf, a.ctf_correct, a.wiener_tau, a.scale) == ('c.txt', 'flip', 0.02, 2.0)
    with pytest.raises(SystemExit):
        p.parse_args(need + ['--ctf-correct', 'both'])
    p = resolution.build_parser(ctf=True)
    assert sorted(set(_flags(p)) - set(_flags(resolution.build_parser()))) == ['--ctf', '--ctf-correct', '--scale']
    a = p.parse_args(need + ['--ctf', 'c.txt'])
    assert (a.ctf, a.ctf_correct, a.scale) == ('c.txt', 'flip', 1)
    with pytest.raises(SystemExit):
        p.parse_args(need + ['--ctf', 'c.txt', '--ctf-correct', 'wiener'])
    # the scripts parse the flags
    src_a = open(os.path.join(PKG, 'tvae', 'align.py')).read()
    src_r = open(os.path.join(PKG, 'tvae', 'resolution.py')).read()
    assert 'build_parser(ctf=True).parse_args(argv)' in src_a and 'build_parser(ctf=True).parse_args(argv)' in src_r


def test_ctf_bench_parser():
    spec = importlib.util.spec_from_file_location('ctf_bench', os.path.join(ROOT, 'profiles', 'tools', 'ctf_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert _flags(p) == sorted(['--shapes', '--bank-shapes', '--wiener-shape', '--clusters', '--host-rows', '--reps', '--warmup',
                                '--out', '--tag'])
    a = p.parse_args([])
    assert a.shapes == ['100000x128', '20000x64', '20000x256'] and a.bank_shapes == ['100000x127', '100000x63']
    assert (a.wiener_shape, a.clusters, a.host_rows, a.reps) == ('100000x128', 10, 200, 10)
    assert mod.parse_shape('20000x64') == (20000, 64)
    assert mod.issued_flop(1, 128) == 2 * 32 * 32 * 2 * (12 * 64 * 2 + 12 * 64 * 4 * 2 + 16 * 33 * 2)


# ---- header, binding, queries ----------------------------------------------------------------------------------------------
NEW_CALLS = {'tvae_ctf_eval': 'ppiii', 'tvae_fourier_filter': 'plpplppliii', 'tvae_ctf_power': 'pppppiii'}
NEW_QUERIES = {'tvae_fourier_filter_ws_floats': ('ii', 'l')}


def test_header_and_binding_of_the_new_entry_points():
    from tvae import _cluster_lib as CL, _lib
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
    for name, sig in NEW_CALLS.items():
        assert CL.SIGNATURES[name] == sig
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[-1].startswith('tvae_stream_t') and len(args) - 1 == len(sig)
        for pos, (a, c) in enumerate(zip(args[:-1], sig)):
            assert ('*' in a) == (c == 'p') and a.startswith({'p': ('const ', 'float', 'int', 'double'), 'f': 'float ',
                                                               'l': 'long ', 'i': 'int '}[c]), (name, a)
            assert ('double*' in a) == ((name, pos) in _lib._F64_OK), (name, pos, a)
    for name, (sig, ret) in NEW_QUERIES.items():
        assert CL.QUERIES[name] == (sig, ret)
        m = re.search(r'\b(int|long)\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m and m.group(1) == {'i': 'int', 'l': 'long'}[ret]
        assert all(a.strip().startswith('int ') for a in m.group(2).split(',')) and len(m.group(2).split(',')) == len(sig)
    L = CL.lib()
    assert L.tvae_cluster_abi_version() == CL.ABI_VERSION == 1
    for name in list(NEW_CALLS) + list(NEW_QUERIES):
        assert hasattr(L, name), name
    flat = ' '.join(hdr.split())
    assert 'Astigmatism (dfdiff, dfang) is IGNORED' in flat and 'reduced to t - rint(t) in fp64' in flat
    assert '8 2^-24 (|c0| + |c1|)' in flat and 'n <= 128: the spectrum stays in LDS' in flat


def test_query():
    from tvae import _cluster_lib as CL
    for B, n in [(1, 2), (5, 31), (7, 128), (1 << 24, 64)]:
        assert CL.query('tvae_fourier_filter_ws_floats', B, n) == 2
    for B, n in [(1, 129), (5, 130), (3, 255), (2, 1024), (1 << 24, 1024)]:
        assert CL.query('tvae_fourier_filter_ws_floats', B, n) == B * 4 * n * ((n // 2 + 1) | 1)
    for bad in [(0, 8), (-1, 8), ((1 << 24) + 1, 8), (4, 0), (4, 1), (4, 1025), (4, -3)]:
        assert CL.query('tvae_fourier_filter_ws_floats', *bad) == 0, bad


def test_cpu_tensors_are_refused():
    from tvae import ctf
    x = torch.zeros(2, 8, 8)
    with pytest.raises(ctf.TvaeHipError):
        ctf.filter_stack(x, coef=np.zeros((2, 5)))
    with pytest.raises(ctf.TvaeHipError):
        ctf.filter_stack(x, planes=torch.ones(8, 5))
    with pytest.raises(ctf.TvaeHipError):
        ctf.class_averages_ctf(torch.zeros(2, 1, 8, 8), torch.zeros(2), torch.zeros(2, 2), np.zeros(2, int), np.zeros((2, 5)))
