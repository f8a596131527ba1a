"""Particle preprocessing on the GPU: tvae_image_resample and tvae_image_normalize behind their C ABI (every call under guard
bands with replay, outputs and workspace filled with a sentinel) against the fp64 restatement tests/image_ref.py, then
tvae.image, the src.image drop-in and preprocess_particles.py against the goldens of the reference's src/image.py.

Resample, against fp64 on the SAME fp32 tables and pixels (converted to double): two chained fp32 dot products of lengths
M and N, the scale, the subtraction and the store, per element and a priori:
    |got - ref| <= (M + N + 8) 2^-24 |scale| (|Ar| |X| |Br| + |Ai| |X| |Bi|).
Normalize, against fp64 on the same fp32 pixels: the one rounding of the result to fp32 (twice over) and the fp64 sums of at
most 2^20 terms (2^-33 relative, with 8 x slack) acting on the numerator and, through mu, on it again:
    |got - ref| <= 2 * 2^-24 |ref| + 2^-30 (|x - mu| + |mu|) / sigma,        stats to 2^-30 relative.
Against the GOLDENS (fp64 inputs the host side rounds to fp32 first) the input's rounding is added, see the tests.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guardband
import image_ref
from conftest import GOLDEN, PKG, load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 2.0 ** -24
SENT_F = -12345.5
B_IMG = 5
# (M, N) -> (m, n): the smallest sizes that cross each edge of the kernel -- one partial tile; reductions that are no
# multiple of 16; more than one chunk of 64 columns (65, 130); two row tiles and the 128-wide column tile (96 x 80); three
# chunks with tails and a 33-wide output; a single output pixel; two 128-wide column tiles next to two row tiles (70 x 135)
SHAPES = [((16, 16), (8, 8)), ((33, 31), (7, 10)), ((65, 65), (32, 32)), ((96, 80), (96, 80)), ((130, 130), (33, 33)),
          ((8, 8), (1, 1)), ((140, 150), (70, 135))]
KINDS = ('real', 'random', 'null')


@pytest.fixture(scope='module', autouse=True)
def _own_guarded_names():
    """The closed-coverage assertion of test_hip_primitives.py compares guardband.GUARDED_NAMES with tvae._lib.SIGNATURES:
    the names this file adds are taken out again."""
    before = set(guardband.GUARDED_NAMES)
    yield
    from tvae import _cluster_lib
    guardband.GUARDED_NAMES.difference_update(set(_cluster_lib.SIGNATURES) - before)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV, dtype).contiguous()


# ---- the C ABI under guard bands ---------------------------------------------------------------------------------------------
def run_resample(X, tabs, window, m, n, scale, B=None):
    """tvae_image_resample into a sentinel-filled output -> numpy [B][m][n]."""
    from tvae import _cluster_lib as CL
    _, H, W = X.shape
    B = X.shape[0] if B is None else B
    r0, c0, M, N = window
    out = torch.full((max(B, 1), max(m, 1), max(n, 1)), SENT_F, device=DEV)
    try:
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_image_resample', _dev(X), *[_dev(t) for t in tabs], out, B, H, W, r0, c0, M, N, m, n, scale)
    finally:
        run_resample.last = out.cpu().numpy()
    return out.cpu().numpy()


def run_normalize(X, radius, inplace=False, B=None, n=None, m=None, ws_short=0):
    """tvae_image_normalize with sentinel-filled output, statistics and workspace -> (out, stats) as numpy."""
    from tvae import _cluster_lib as CL
    B = X.shape[0] if B is None else B
    n = X.shape[1] if n is None else n
    m = X.shape[2] if m is None else m
    wsf = CL.query('tvae_image_normalize_ws_floats', *X.shape)
    assert wsf > 0 and wsf % 2 == 0
    ws = torch.full((wsf // 2,), SENT_F, dtype=torch.float64, device=DEV).view(torch.float32)
    x = _dev(X)
    out = x if inplace else torch.full(X.shape, SENT_F, device=DEV)
    stats = torch.full((X.shape[0], 2), SENT_F, dtype=torch.float64, device=DEV)
    try:
        with guardband.GuardedCalls(replay=True):
            CL.call('tvae_image_normalize', x, out, stats, ws, wsf - ws_short, B, n, m, radius)
    finally:
        run_normalize.last = (out.cpu().numpy(), stats.cpu().numpy(), ws.cpu().numpy())
    return out.cpu().numpy(), stats.cpu().numpy()


def resample_bound(X, tabs, scale, M, N):
    return (M + N + 8) * EPS * image_ref.sandwich_bound(X, *tabs, scale)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """Inputs, the fp64 reference (computed once, never modified), the a-priori bound and the guarded GPU result."""
    from tvae import tables
    (M, N), (m, n) = shape
    rng = np.random.default_rng([M, N, m, n, KINDS.index(kind)])
    X = (rng.standard_normal((B_IMG, M, N)) + 0.5).astype(np.float32)
    if kind == 'real':
        tabs, scale = tables.resample_tables(M, N, m, n), 1.0 / (M * N)
    else:
        tabs = [rng.standard_normal(s).astype(np.float32) for s in ((m, M), (m, M), (N, n), (N, n))]
        scale = 0.37
        if kind == 'null':
            tabs[1] = tabs[3] = None
    scale = float(np.float32(scale))                                      # the factor the kernel gets
    ref = image_ref.sandwich(X, *tabs, scale)
    got = run_resample(X, tabs, (0, 0, M, N), m, n, scale)
    for a in (X, ref):
        a.setflags(write=False)
    return dict(X=X, tabs=tabs, scale=scale, ref=ref, bound=resample_bound(X, tabs, scale, M, N), got=got)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_resample_against_fp64(shape, kind):
    c = case(shape, kind)
    assert c['got'].shape == c['ref'].shape and np.isfinite(c['got']).all()
    err = np.abs(c['got'] - c['ref'])
    print('max error / bound: %.3f' % (err / c['bound']).max())
    assert (err <= c['bound']).all()
    if kind == 'real':                                                    # ... and the real tables do downsample
        want = image_ref.downsample(c['X'], shape[1])
        (M, N) = shape[0]
        assert (np.abs(c['got'] - want) <= (M + N + 11) / (M + N + 8) * c['bound'] + 1e-12).all()


@pytest.mark.parametrize('kind', ('real', 'random'))
def test_resample_window_of_a_larger_frame(kind):
    """A 36 x 36 window at (3, 5) of a 40 x 44 frame -> 12 x 12; every pixel outside the window is 1e30, so a single read
    outside it breaks the bound."""
    from tvae import tables
    rng = np.random.default_rng(77)
    H, W, r0, c0, M, N, m, n = 40, 44, 3, 5, 36, 36, 12, 12
    X = np.full((B_IMG, H, W), 1e30, dtype=np.float32)
    X[:, r0:r0 + M, c0:c0 + N] = rng.standard_normal((B_IMG, M, N))
    if kind == 'real':
        tabs, scale = tables.resample_tables(M, N, m, n), float(np.float32(1.0 / (M * N)))
    else:
        tabs, scale = [rng.standard_normal(s).astype(np.float32) for s in ((m, M), (m, M), (N, n), (N, n))], 1.0
    win = X[:, r0:r0 + M, c0:c0 + N]
    got = run_resample(X, tabs, (r0, c0, M, N), m, n, scale)
    assert (np.abs(got - image_ref.sandwich(win, *tabs, scale)) <= resample_bound(win, tabs, scale, M, N)).all()
    # the window as a frame of its own: the same bits
    assert np.array_equal(got, run_resample(np.ascontiguousarray(win), tabs, (0, 0, M, N), m, n, scale))


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3], SHAPES[6]], ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_resample_is_reproducible_and_independent_of_the_batch(shape):
    (M, N), (m, n) = shape
    for kind in ('random', 'null'):
        c = case(shape, kind)
        again = run_resample(c['X'], c['tabs'], (0, 0, M, N), m, n, c['scale'])
        assert np.array_equal(again, c['got'])
        for b in (0, 3):
            one = run_resample(c['X'][b:b + 1], c['tabs'], (0, 0, M, N), m, n, c['scale'])
            assert np.array_equal(one[0], c['got'][b]), (kind, b)


def test_resample_rejects_unsupported_arguments():
    from tvae._lib import TvaeHipError
    rng = np.random.default_rng(5)
    X = rng.standard_normal((2, 20, 24)).astype(np.float32)

    def tabs(M, N, m, n):
        return [np.ones(s, dtype=np.float32) for s in ((m, M), (m, M), (N, n), (N, n))]

    bad = [
        dict(window=(0, 0, 8, 8), m=9, n=4, tabs=tabs(8, 8, 9, 4)),                     # m > M
        dict(window=(0, 0, 8, 8), m=4, n=9, tabs=tabs(8, 8, 4, 9)),                     # n > N
        dict(window=(13, 0, 8, 8), m=4, n=4, tabs=tabs(8, 8, 4, 4)),                    # the window leaves the frame below
        dict(window=(0, 17, 8, 8), m=4, n=4, tabs=tabs(8, 8, 4, 4)),                    # ... and on the right
        dict(window=(-1, 0, 8, 8), m=4, n=4, tabs=tabs(8, 8, 4, 4)),
        dict(window=(0, 0, 8, 8), m=0, n=4, tabs=tabs(8, 8, 1, 4)),
        dict(window=(0, 0, 8, 8), m=4, n=4, tabs=tabs(8, 8, 4, 4), B=0),                # B = 0
        dict(window=(0, 0, 8, 8), m=4, n=4, tabs=tabs(8, 8, 4, 4)[:1] + [None] + tabs(8, 8, 4, 4)[2:]),   # Ai alone NULL
    ]
    for kw in bad:
        with pytest.raises(TvaeHipError, match='hipError_t 1'):
            run_resample(X, kw['tabs'], kw['window'], kw['m'], kw['n'], 1.0, B=kw.get('B'))
        assert (run_resample.last == SENT_F).all()
    # a size above 1024: the frame really is that large, only the limit is in the way
    big = np.zeros((1, 1025, 8), dtype=np.float32)
    with pytest.raises(TvaeHipError, match='hipError_t 1'):
        run_resample(big, tabs(1025, 8, 4, 4), (0, 0, 1025, 8), 4, 4, 1.0)
    with pytest.raises(TvaeHipError, match='hipError_t 1'):
        run_resample(big.reshape(1, 8, 1025), tabs(8, 1025, 4, 4), (0, 0, 8, 1025), 4, 4, 1.0)
    assert (run_resample.last == SENT_F).all()
    # (the guard's 'rejected' check has also compared every tensor of a refused call with its contents before the call)


# ---- normalize -------------------------------------------------------------------------------------------------------------
NORM_CASES = [((7, 9), None), ((7, 9), 3.0), ((64, 64), None), ((64, 64), 20.5), ((130, 70), None), ((130, 70), 41.25)]


def normalize_bounds(X, ref, stats):
    mu, sd = stats[:, 0, None, None], stats[:, 1, None, None]
    return 2 * EPS * np.abs(ref) + 2.0 ** -30 * (np.abs(X.astype(np.float64) - mu) + np.abs(mu)) / sd


@pytest.mark.parametrize('inplace', (False, True), ids=('out', 'inplace'))
@pytest.mark.parametrize('shape,radius', NORM_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_normalize_against_fp64(shape, radius, inplace):
    """Mean 1000, spread 1: the sum-of-squares form of sigma would lose every digit in fp32 and half of them in fp64."""
    n, m = shape
    rng = np.random.default_rng(n * 1000 + m)
    X = (1000.0 + rng.standard_normal((3, n, m))).astype(np.float32)
    X[1] = (0.25 * rng.standard_normal((n, m)) - 3.0).astype(np.float32)
    ref, ref_stats = image_ref.normalize(X, radius)
    got, stats = run_normalize(X, 0.0 if radius is None else radius, inplace)
    assert (np.abs(stats - ref_stats) <= 2.0 ** -30 * np.abs(ref_stats)).all(), (stats, ref_stats)
    err, bound = np.abs(got - ref), normalize_bounds(X, ref, ref_stats)
    print('max error / bound: %.3f' % (err / bound).max())
    assert (err <= bound).all()
    # the background ring of the result: mean 0, standard deviation 1
    ring = got[:, image_ref.ring_mask(n, m, radius)].astype(np.float64)
    assert np.abs(ring.mean(1)).max() < 1e-3 and np.abs(ring.std(1) - 1).max() < 1e-3
    # a negative radius is the default as well; an image's result does not depend on the others
    if not inplace:
        if radius is None:
            assert np.array_equal(run_normalize(X, -2.0)[0], got)
        one, one_stats = run_normalize(X[1:2], 0.0 if radius is None else radius)
        assert np.array_equal(one[0], got[1]) and np.array_equal(one_stats[0], stats[1])


def test_normalize_degenerate_masks():
    gold = load_golden('image_ref')
    got, stats = run_normalize(gold['norm_empty_x'].astype(np.float32), float(gold['norm_empty_radius']))
    assert np.isnan(gold['norm_empty_y']).all() and np.isnan(got).all() and np.isnan(stats).all()
    x, want = gold['norm_const_x'].astype(np.float32), gold['norm_const_y']
    got, stats = run_normalize(x, 0.0)
    assert not np.isfinite(want).any() and not np.isfinite(got).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    assert (stats[:, 0] == 2.5).all() and (stats[:, 1] == 0).all()


def test_normalize_rejects_unsupported_arguments():
    from tvae._lib import TvaeHipError
    X = np.random.default_rng(9).standard_normal((2, 8, 8)).astype(np.float32)
    for kw in (dict(radius=float('nan')), dict(radius=float('inf')), dict(radius=0.0, B=0), dict(radius=0.0, n=1025),
               dict(radius=0.0, m=0), dict(radius=0.0, ws_short=1)):
        with pytest.raises(TvaeHipError, match='hipError_t 1'):
            run_normalize(X, **kw)
        out, stats, ws = run_normalize.last
        assert (out == SENT_F).all() and (stats == SENT_F).all()
        assert np.array_equal(ws.view(np.float64), np.full(ws.size // 2, SENT_F))


# ---- host side -------------------------------------------------------------------------------------------------------------
def test_host_functions_reproduce_the_goldens():
    """Against the reference's fp64 results.  The host side rounds the fp64 input and the fp64 tables to fp32 first: one more
    2^-24 for the pixels and one for each table, relative to the same sum of magnitudes, on top of the kernel's bound."""
    from tvae import image, tables
    import src.image as drop_in
    gold = load_golden('image_ref')
    for k in range(10):
        x, want = gold[f'down{k}_x'], gold[f'down{k}_y']
        m, n = (int(v) for v in gold[f'down{k}_shape'])
        M, N = x.shape[-2:]
        tol = (M + N + 11) * EPS * image_ref.sandwich_bound(x, *tables.resample_tables_f64(M, N, m, n), 1.0 / (M * N)) + 1e-12
        got = drop_in.downsample(x, shape=(m, n))
        assert got.dtype == np.float64 and got.shape == want.shape and (np.abs(got - want) <= tol).all(), k
        got32 = drop_in.downsample(x.astype(np.float32), shape=(m, n))
        assert got32.dtype == np.float32 and np.array_equal(got32, got.astype(np.float32))
        t = image.downsample(torch.from_numpy(x).to(DEV), shape=(m, n))
        assert t.dtype == torch.float32 and t.is_cuda and np.array_equal(t.cpu().numpy(), got32)
    x, want = gold['downf_x'], gold['downf_y']
    tol = (16 + 12 + 11) * EPS * image_ref.sandwich_bound(x, *tables.resample_tables_f64(16, 12, 6, 4), 1.0 / (16 * 12)) + 1e-12
    assert (np.abs(drop_in.downsample(x, 2.5) - want) <= tol).all()
    assert (np.abs(drop_in.downsample(x[0], factor=2.5) - want[0]) <= tol[0]).all()          # a single 2-D image
    # normalize: rounding the input moves a pixel and mu by at most u = 2^-24 max |x| each and sigma by at most u
    for k in range(4):
        x, want, radius = gold[f'norm{k}_x'], gold[f'norm{k}_y'], float(gold[f'norm{k}_radius'])
        radius = None if np.isnan(radius) else radius
        ref, stats = image_ref.normalize(x, radius)
        u = EPS * np.abs(x).max() / stats[:, 1, None, None]
        tol = normalize_bounds(x.astype(np.float32), ref, stats) + 1.01 * u * (2 + np.abs(ref)) + 1e-12
        got = drop_in.normalize(x) if radius is None else drop_in.normalize(x, radius)
        assert got.dtype == np.float64 and (np.abs(got - want) <= tol).all(), k
        got32 = drop_in.normalize(x.astype(np.float32), radius)
        assert got32.dtype == np.float32 and np.array_equal(got32, got.astype(np.float32))
        t, st = image.normalize(torch.from_numpy(x).to(DEV), radius, return_stats=True)
        assert np.array_equal(t.cpu().numpy(), got32) and st.dtype == torch.float64 and st.shape == (2, 2)
        assert (np.abs(st.cpu().numpy() - stats) <= 2 * EPS * np.abs(x).max()).all()
    x = torch.from_numpy(gold['crop_x']).to(DEV)
    v = image.crop(x, 4)
    assert np.array_equal(v.cpu().numpy(), gold['crop_y']) and v.data_ptr() == x[0, 2:, 3:].data_ptr()
    with pytest.raises(image.TvaeHipError):
        image.normalize(x, radius=0.0)
    assert len({k[:4] for k in image._DEVICE_TABLES}) == len(image._DEVICE_TABLES) >= 10     # one upload per shape


def test_preprocess_particles_script(tmp_path):
    """The command line on the reference-written stack (5 images of 6 x 7, pixel size 1.5 x 2.5): crop to 6 x 6, downsample
    to 4 x 3, normalize, two images per trip -- bit for bit tvae.image applied step by step to the whole stack at once."""
    from src import mrc
    from tvae import image
    stack = os.path.join(GOLDEN, 'stack_ref.mrcs')
    raw, header = mrc.open_stack(stack)
    assert raw.shape == (5, 6, 7) and (header.xlen, header.ylen) == (1.5, 2.5)
    out = str(tmp_path / 'small.mrcs')
    cmd = [sys.executable, os.path.join(PKG, 'preprocess_particles.py'), '--stack', stack, '--out', out, '--crop', '6',
           '--shape', '4', '3', '--normalize', '--chunk', '2']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    got, h = mrc.open_stack(out)
    x = image.crop(torch.from_numpy(np.array(raw)).to(DEV), 6).contiguous()
    want, stats = image.normalize(image.downsample(x, shape=(4, 3)), return_stats=True)
    assert got.shape == (5, 4, 3) and got.dtype == np.float32 and h.mode == 2
    assert np.array_equal(np.array(got), want.cpu().numpy())
    assert np.array_equal(np.load(out + '.stats.npy'), stats.cpu().numpy())
    assert (h.xlen / h.mx, h.ylen / h.my) == (1.5 * 6 / 3, 2.5 * 6 / 4)
    # a factor instead of a shape, no normalisation: no statistics file
    out2 = str(tmp_path / 'half.mrcs')
    r = subprocess.run(cmd[:2] + ['--stack', stack, '--out', out2, '--downsample', '2'], capture_output=True, text=True,
                       timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    got2, h2 = mrc.open_stack(out2)
    want2 = image.downsample(torch.from_numpy(np.array(raw)).to(DEV), 2)
    assert got2.shape == (5, 3, 3) and np.array_equal(np.array(got2), want2.cpu().numpy())
    assert not os.path.exists(out2 + '.stats.npy') and (h2.xlen / h2.mx, h2.ylen / h2.my) == (1.5 * 7 / 3, 2.5 * 6 / 3)
