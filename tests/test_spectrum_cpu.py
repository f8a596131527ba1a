"""Radial spectra, the part that needs no GPU: the header and the binding of the six new entry points and the built library,
the ring table against the FRC's, the host arithmetic of tvae.spectrum (ring counts, the window, the whitening profile, the
FRC profile), the reference's own normalisation on white noise, the two parsers and the argument errors of the two scripts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import frc_ref
import spectrum_ref
from conftest import PKG, ROOT

NEW_CALLS = {'tvae_ring_power': 'plppliiffii', 'tvae_ring_power_groups': 'pppppiii', 'tvae_radial_filter': 'plpppp' 'l' 'iiii'}
NEW_QUERIES = {'tvae_radial_rings': ('i', 'i'), 'tvae_ring_power_ws_floats': ('ii', 'l'),
               'tvae_radial_filter_ws_floats': ('ii', 'l')}
F64 = {('tvae_ring_power', 2), ('tvae_ring_power_groups', 0), ('tvae_ring_power_groups', 3)}


# ---- header, binding, library ------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_six_names():
    from tvae import _cluster_lib as CL, _lib
    hdr = open(os.path.join(ROOT, 'include', 'tvae_cluster.h')).read()
    start = hdr.index('/* ---- Radial spectra')
    section = hdr[start:hdr.index('/* ---- Eigenimages')]
    declared = re.findall(r'^(?:int|long)\s+(tvae_\w+)\s*\(', section, re.M)
    assert sorted(declared) == sorted(list(NEW_CALLS) + list(NEW_QUERIES))
    assert hdr.index('/* ---- CTF:') < start
    for name in declared:
        assert not any(w in name for w in ('refine', 'classify', 'posterior', 'weighted'))
    for name, sig in NEW_CALLS.items():
        assert CL.SIGNATURES[name] == sig
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[-1].startswith('tvae_stream_t') and len(args) - 1 == len(sig), name
        for pos, (a, c) in enumerate(zip(args[:-1], sig)):
            assert ('*' in a) == (c == 'p') and a.startswith({'p': ('const ', 'float', 'int', 'double'), 'f': 'float ',
                                                               'l': 'long ', 'i': 'int '}[c]), (name, a)
            assert ('double*' in a) == ((name, pos) in F64) == ((name, pos) in _lib._F64_OK), (name, pos, a)
    for name, (sig, ret) in NEW_QUERIES.items():
        assert CL.QUERIES[name] == (sig, ret)
        m = re.search(r'\b(int|long)\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m and m.group(1) == {'i': 'int', 'l': 'long'}[ret]
        assert all(a.strip().startswith('int ') for a in m.group(2).split(',')) and len(m.group(2).split(',')) == len(sig)
    flat = ' '.join(section.replace('\n *', ' ').split())
    assert "A g outside [0, G) makes that plane's output exact zeros" in flat
    assert 'bit for bit that of tvae_fourier_filter' in flat and 'ascending ky index, then ascending kx' in flat


def test_library_exports_them_and_the_abi_version_stays():
    from tvae import _cluster_lib as CL
    L = CL.lib()
    assert L.tvae_cluster_abi_version() == CL.ABI_VERSION == 1
    for name in list(NEW_CALLS) + list(NEW_QUERIES):
        assert hasattr(L, name), name
        assert name in CL.exported_symbols()


def test_queries():
    from tvae import _cluster_lib as CL
    for q in ('tvae_ring_power_ws_floats', 'tvae_radial_filter_ws_floats'):
        for B, n in [(1, 2), (5, 31), (7, 128), (1 << 24, 64)]:
            assert CL.query(q, B, n) == 2
        for B, n in [(1, 129), (5, 130), (2, 1024)]:
            assert CL.query(q, B, n) == B * 4 * n * ((n // 2 + 1) | 1) == CL.query('tvae_fourier_filter_ws_floats', B, n)
        for bad in [(0, 8), (-1, 8), ((1 << 24) + 1, 8), (4, 0), (4, 1), (4, 1025), (4, -3)]:
            assert CL.query(q, *bad) == 0, bad
    for bad in (-1, 0, 1, 1025):
        assert CL.query('tvae_radial_rings', bad) == 0
    assert [CL.query('tvae_radial_rings', n) for n in (2, 3, 64, 65, 128, 129, 1024)] == [2, 2, 46, 46, 92, 92, 725]


# ---- rings ---------------------------------------------------------------------------------------------------------------------
def test_ring_table_and_ring_count():
    from tvae import _cluster_lib as CL, spectrum
    for n in range(2, 131):
        h = n // 2
        idx = frc_ref.ring_index(n)
        Rr = 1 + frc_ref.ring_of(h, h)
        assert CL.query('tvae_radial_rings', n) == spectrum.radial_rings(n) == spectrum_ref.rings(n) == Rr, n
        assert idx[:, :h + 1].max() + 1 == Rr == idx.max() + 1, n           # the largest ring of the half spectrum, plus one
        tab = spectrum.ring_table(n)
        assert np.array_equal(tab, idx), n                                   # rings 0 .. n / 2 are the FRC's, corners beyond
        cnt = spectrum.ring_counts(n)
        assert cnt.dtype == np.float64 and cnt.shape == (Rr,) and cnt.sum() == n * n and (cnt > 0).all(), n
        assert np.array_equal(cnt, spectrum_ref.ring_counts(n))
    with pytest.raises(spectrum.TvaeHipError):
        spectrum.radial_rings(1)


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (8, 33, 64))
def test_window_is_the_reference_window(n):
    from tvae import spectrum
    for radius, edge in ((None, 0.0), (0.0, 3.0), (0.3 * n, 0.15 * n), (0.4 * n, 0.0)):
        for bg in (True, False):
            assert np.array_equal(spectrum.window(n, radius, edge, bg), spectrum_ref.window(n, radius, edge, bg)), (radius, bg)
    w = spectrum.window(n, 0.3 * n, 0.15 * n, True)
    assert w.min() == 0.0 and w.max() == 1.0 and w[n // 2, n // 2] == 0.0 and w[0, 0] == 1.0


def test_reference_reads_white_noise_as_its_variance():
    """The normalisation: white noise of variance s^2 reads s^2 on every ring, to the scatter of a ring's mean over 64 planes
    (a ring of m coefficients: relative scatter 1 / sqrt(64 m) without a window, wider by the window's correlation)."""
    n, s = 32, 1.7
    rng = np.random.default_rng(1)
    X = s * rng.standard_normal((64, n, n))
    for radius, edge, bg in ((None, 0.0, True), (0.3 * n, 0.15 * n, True), (0.3 * n, 0.15 * n, False)):
        raw = spectrum_ref.power(X, radius, edge, bg, demean=False)
        got = spectrum_ref.normalised(raw, n, radius, edge, bg).mean(0)
        m = spectrum_ref.ring_counts(n)
        assert (np.abs(got / s ** 2 - 1) <= 8 / np.sqrt(64 * m)).all(), (radius, bg)
    # the float32 restatement agrees with fp64 to a few 1e-6 of every ring's power
    raw = spectrum_ref.power(X[:4], 0.3 * n, 0.15 * n, True, True)
    f32 = spectrum_ref.power_f32(X[:4].astype(np.float32), 0.3 * n, 0.15 * n, True, True)
    assert (np.abs(f32 - raw)[:, 1:] <= 1e-5 * raw[:, 1:]).all()


@pytest.mark.parametrize('n', (2, 3, 8, 31, 33, 64, 65, 96, 127, 128, 129))
def test_reference_alone_meets_the_cap_of_every_gpu_case(n):
    """Every case of test_spectrum_gpu.py::test_power_against_fp64, built without the kernel: a seed is found at which the
    a-priori bound (a) is at most 1e-2 of the reference's own ring power on every ring r >= 1 of every plane, and the limit
    (b) is positive and nowhere above the one figure of test_ctf_gpu.py's rule."""
    import test_spectrum_gpu as G
    assert G.SIZES == (2, 3, 8, 31, 33, 64, 65, 96, 127, 128, 129)
    for name in sorted(G.VARIANTS):
        if n == 2 and name == 'hard-bg-demean':               # an empty window: the NaN case of the GPU file
            continue
        c = G.case_inputs(n, name)
        first = 1 if c['args'][3] else 0
        ref, bound, limit = c['ref'], c['bound'], c['limit']
        assert ref.shape == bound.shape == limit.shape == (G.B_IMG, spectrum_ref.rings(n))
        assert (ref[:, 1:] > 0).all() and (bound[:, 1:] <= 1e-2 * ref[:, 1:]).all(), (n, name, c['seed'])
        assert (limit[:, first:] > 0).all(), (n, name)
        f32 = spectrum_ref.power_f32(c['X'], *c['args'])
        assert (limit[:, first:] <= 8 * np.abs(f32 - ref)[:, first:].max()).all()          # the rule of test_ctf_gpu.py, and no more


def test_whitening_profile():
    from tvae import spectrum
    n = 64
    cnt = spectrum.ring_counts(n)
    r = np.arange(cnt.size)
    spec = np.stack([4.0 / (1 + 0.1 * r) ** 2, np.full(cnt.size, 9.0)])
    H = spectrum.whitening_profile(spec, n=n)
    assert H.shape == spec.shape and H.dtype == np.float64
    assert np.allclose((cnt * H * H).sum(1), n * n, rtol=1e-13)            # unit white noise keeps unit variance
    assert np.allclose(H[1], 1.0, rtol=1e-13)                             # a flat spectrum: the identity
    assert np.allclose(H[0] ** 2 * spec[0], (H[0] ** 2 * spec[0])[0], rtol=1e-12)        # H^2 spec is flat
    assert np.array_equal(spectrum.whitening_profile(spec), H)            # the default n is the even one
    assert np.array_equal(spectrum.whitening_profile(spec[0], n=n), H[0])
    # the floor: a ring of no power does not blow up
    hole = spec[0].copy()
    hole[10] = 0.0
    Hh = spectrum.whitening_profile(hole, floor=1e-2, n=n)
    assert np.isfinite(Hh).all() and np.isclose(Hh[10] / Hh[0], np.sqrt(hole[0] / (1e-2 * np.median(hole))))
    for bad in (dict(spec=np.ones(3), n=n), dict(spec=spec, floor=0.0), dict(spec=np.ones(47))):      # (47 rings: no even n)
        with pytest.raises(ValueError):
            spectrum.whitening_profile(**bad)
    assert spectrum.whitening_profile(np.ones(92), n=129).shape == (92,)


def test_frc_profile():
    from tvae import spectrum
    n = 33
    R, Rr = n // 2 + 1, spectrum_ref.rings(n)
    f = np.linspace(1.0, 0.2, R)
    f[9], f[12] = 0.1, -0.3                                              # a dip below the threshold at ring 9, a negative value
    cref = spectrum.frc_profile(f, n)
    assert cref.shape == (Rr,) and np.allclose(cref[:9], np.sqrt(2 * f[:9] / (1 + f[:9])))
    assert (cref[9:] == 0).all()                                         # a monotone cut: the curve rises again, the filter does not
    hard = spectrum.frc_profile(f, n, 'hard')
    assert (hard[:9] == 1).all() and (hard[9:] == 0).all()
    # no ring below the threshold: FRC < 0 gives 0 under 'cref', the corner rings are 0 unless asked for
    low = spectrum.frc_profile(f, n, 'cref', threshold=-1.0)
    assert low[12] == 0 and low[9] > 0 and (low[R:] == 0).all() and low[R - 1] > 0
    kept = spectrum.frc_profile(f, n, 'hard', threshold=-1.0, corners=True)
    assert (kept == 1).all()
    # ring 0 is never the cut; a batch of curves keeps its leading axes
    g = np.stack([f, np.r_[-1.0, np.ones(R - 1)]])
    both = spectrum.frc_profile(g[:, None], n, 'hard')
    assert both.shape == (2, 1, Rr) and (both[1, 0, :R] == 1).all() and np.array_equal(both[0, 0], hard)
    for bad in (dict(frc=f[:-1], n=n), dict(frc=f, n=n, kind='soft')):
        with pytest.raises(ValueError):
            spectrum.frc_profile(**bad)


def test_cpu_tensors_are_refused():
    from tvae import spectrum
    x = torch.zeros(2, 8, 8)
    for call in (lambda: spectrum.ring_power(x), lambda: spectrum.radial_filter(x, np.ones(6)),
                 lambda: spectrum.whiten(x), lambda: spectrum.filter_averages(x, np.ones((2, 5))),
                 lambda: spectrum.group_power(torch.zeros(2, 6, dtype=torch.float64))):
        with pytest.raises(spectrum.TvaeHipError, match='no CPU fallback'):
            call()


# ---- the two command lines -----------------------------------------------------------------------------------------------------
def _snapshot(parser):
    return [(tuple(a.option_strings), a.dest, a.default, getattr(a.type, '__name__', None),
             list(a.choices) if a.choices else None, a.required) for a in parser._actions if a.dest != 'help']


def test_parsers():
    from tvae import spectrum
    assert _snapshot(spectrum.build_parser('whiten')) == [
        (('--stack',), 'stack', None, None, None, True),
        (('--out',), 'out', None, None, None, True),
        (('--groups',), 'groups', None, None, None, False),
        (('--mask-radius',), 'mask_radius', None, 'float', None, False),
        (('--mask-edge',), 'mask_edge', None, 'float', None, False),
        (('--floor',), 'floor', 1e-3, 'float', None, False),
        (('--chunk',), 'chunk', 4096, 'int', None, False),
        (('--interp',), 'interp', 'linear', None, ['linear', 'nearest'], False),
        (('-d', '--device'), 'device', 0, 'int', None, False)]
    assert _snapshot(spectrum.build_parser('filter')) == [
        (('--averages',), 'averages', None, None, None, True),
        (('--frc',), 'frc', None, None, None, True),
        (('--kind',), 'kind', 'cref', None, ['cref', 'hard'], False),
        (('--threshold',), 'threshold', 0.143, 'float', None, False),
        (('--apix',), 'apix', None, 'float', None, False),
        (('--out-dir',), 'out_dir', '.', None, None, False),
        (('-d', '--device'), 'device', 0, 'int', None, False)]
    with pytest.raises(ValueError):
        spectrum.build_parser('other')
    for script, tool in (('whiten_particles.py', "run(tool='whiten')"), ('filter_class_averages.py', "run(tool='filter')")):
        src = open(os.path.join(PKG, script)).read()
        assert 'from tvae.spectrum import run' in src and tool in src


def test_command_line_argument_errors(tmp_path):
    from tvae import spectrum
    for tool, argv in (('whiten', ['--stack', 's.mrcs']), ('whiten', ['--stack', 's.mrcs', '--out', 'o.mrcs', '--interp', 'cubic']),
                       ('filter', ['--averages', 'a.npy']), ('filter', ['--averages', 'a.npy', '--frc', 'f.npy', '--kind', 'soft'])):
        with pytest.raises(SystemExit):
            spectrum.build_parser(tool).parse_args(argv)
    np.save(tmp_path / 'g.npy', np.zeros(4))
    with pytest.raises(SystemExit, match='--groups must hold integers'):
        spectrum.run(['--stack', 's.mrcs', '--out', 'o.mrcs', '--groups', str(tmp_path / 'g.npy')], 'whiten')
    with pytest.raises(SystemExit, match='--floor = 0.0 must be positive'):
        spectrum.run(['--stack', 's.mrcs', '--out', 'o.mrcs', '--floor', '0'], 'whiten')
    with pytest.raises(SystemExit, match='the MI355X build has no CPU compute path'):
        spectrum.run(['--stack', 's.mrcs', '--out', 'o.mrcs', '-d', '-1'], 'whiten')
    np.save(tmp_path / 'a.npy', np.zeros((3, 1, 8, 8), np.float32))
    np.save(tmp_path / 'f.npy', np.zeros((3, 1, 4)))
    with pytest.raises(SystemExit, match='does not belong to --averages'):
        spectrum.run(['--averages', str(tmp_path / 'a.npy'), '--frc', str(tmp_path / 'f.npy')], 'filter')
    np.save(tmp_path / 'f.npy', np.zeros((3, 1, 5)))
    with pytest.raises(SystemExit, match='the MI355X build has no CPU compute path'):
        spectrum.run(['--averages', str(tmp_path / 'a.npy'), '--frc', str(tmp_path / 'f.npy'), '-d', '-1'], 'filter')
    # the script itself: a missing required flag ends it with argparse's status
    r = subprocess.run([sys.executable, os.path.join(PKG, 'whiten_particles.py'), '--out', 'o.mrcs'], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and '--stack' in r.stderr
